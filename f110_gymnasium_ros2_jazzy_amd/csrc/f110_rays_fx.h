// f110_rays_fx.h — what the fixed-point ray kernels share (k_rays_fx and k_rays_fxn in
// f110_rays_fx.hip, k_rays_fxs in f110_rays_fxs.hip): the fixed-point cell index of the row-major
// EDT tables, its IEEE fallbacks, the rays' epilogue and the diagnostic wave stamps.
//
// The fixed-point cell index (axis-aligned maps; same results as k_rays_tiled, bit for bit):
//
// xy_2_rc's column is int(x_rot / res) with x_rot = x - orig_x
// (laser_models.py:55-86).  Here one fma puts q = (x - orig_x) / res on a
// 2^-30 fixed-point grid: t = fma(x, inv_res, M - orig_x * inv_res) with
// M = 1.5 * 2^22, so t = M + q lies in [2^22, 2^23) for every on-map q and
// bits [50:30] of t are int(q), bits [29:0] its fraction.  The column, the
// row, the bounds test and a guard band then cost integer ops only, where the
// fp64 form took 2 fp64 subtracts, 2 multiplies, 2 fract, 2 adds, a max, 5
// compares and 2 conversions per lookup.
//
// Error budget (in units of q): the constant's rounding (2^-31), t's rounding
// (2^-31), inv_res's rounding, the reference's own rounding of x - orig_x
// and of x_rot / res (each <= q * 2^-53 <= 2^-32 for q < 2^21): < 2^-29 in
// all.  A lane whose fraction lies within kFxBand * 2^-30 = 2^-28 of an
// integer (either coordinate) takes the exact IEEE path of tiled_cell behind a
// wave-uniform branch; every other lane has the reference's cell and the
// reference's bounds verdict (x_rot >= 0 and x_rot < W * res are decided by
// more than the budget).  Off-map: the sign / exponent test rejects any t
// outside [2^22, 2^23) (NaN and inf included), the column test the rest.
//
// The loop test d > eps is the high word of d != 0: every EDT entry is 0 or
// >= res > eps (checked at f110_create).  Per car, the set-up (beam-index run,
// scan pose, speed, noise counter) is wave-uniform and read with scalar loads.
#pragma once

#include "f110_map.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

template <class T>
__device__ __forceinline__ T ld_const(const T *p) {  // read-only for the kernel: a scalar load when uniform
    return *reinterpret_cast<const __attribute__((address_space(4))) T *>(reinterpret_cast<uintptr_t>(p));
}

__device__ __forceinline__ uint32_t dhi(double v) { return (uint32_t)(__double_as_longlong(v) >> 32); }
__device__ __forceinline__ uint32_t dlo(double v) { return (uint32_t)__double_as_longlong(v); }

// The fixed-point loop's EDT: the row-major table of k_rays_fx / k_rays_fxn
// (FxTable, f110_step_args.h), rows of k1 = wt * 8 bytes: row * k1 + col * 8, and off-map
// indices are clamped into the padding, which holds dt[-1,-1], instead of
// selected.  Measured at 65536 envs: 1.184 vs 1.210 ms for the
// 4x4-tiled table; an inexact f32 8x4-tiled or u16 8x8-tiled table (4x the
// cells per cache line) gained only 2-3 %: the gathers' line footprint is not
// what bounds the loop.
__device__ __forceinline__ uint32_t fx_offset(uint32_t k1, uint32_t row, uint32_t col) {
    return __umul24(row, k1) + (col << 3);
}

__device__ __forceinline__ double fx_load(const void *base, uint32_t off) {
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + off);
}

// tiled_cell's IEEE path as a byte offset of the row-major table (the
// fixed-point path's fallback); oob8: the byte offset of dt[-1,-1]
__device__ __forceinline__ uint32_t exact_offset(const TiledMapView &m, double x, double y, uint32_t oob8) {
    const double xr = x - m.ox, yr = y - m.oy;
    const bool inb = (xr >= 0) & (xr < m.wres) & (yr >= 0) & (yr < m.hres);  // false for NaN
    if (!inb) return oob8;
    int32_t c = (int32_t)(xr / m.res);
    int32_t r = (int32_t)(yr / m.res);
    if (c >= m.W) {  // dt[r, W] is dt[r+1, 0] in the reference's row-major read
        c = 0;
        ++r;
    }
    return r >= m.H ? oob8 : fx_offset((uint32_t)m.wt * 8u, (uint32_t)r, (uint32_t)c);
}

// Loop-invariant state of the fixed-point sphere trace.
struct FxLoop {
    double cxk, cyk, ir, mr;
    uint32_t oobv, W, H, k1;
};

__device__ __forceinline__ FxLoop fx_loop(const RayArgs &a) {
    FxLoop L;
    // the off-map offset and inv_res in VGPRs for the whole trace (opaque
    // copies: the select cannot read an SGPR beside its VCC condition, and the
    // fma's other operand is an SGPR constant, a VOP3 reads one SGPR); the
    // row-major layout carries the off-map byte offset itself in m.oob
    asm volatile("v_mov_b32 %0, %1" : "=v"(L.oobv) : "s"((uint32_t)a.m.oob));
    asm volatile("v_mov_b64 %0, %1" : "=v"(L.ir) : "s"(a.m.inv_res));
    L.cxk = a.fx_cx;
    L.cyk = a.fx_cy;
    L.mr = a.max_range;
    L.W = (uint32_t)a.m.wt - 1u;  // rows of m.wt cells; columns W .. wt-1 and row H hold dt[-1,-1]
    L.H = (uint32_t)a.m.H;
    L.k1 = (uint32_t)a.m.wt * 8u;
    return L;
}

// One iteration of trace_ray's loop (laser_models.py:135-141) for an active
// lane: step, fixed-point cell, EDT lookup.
__device__ __forceinline__ void fx_step(const TiledMapView &m, const FxLoop &L, double &x, double &y, double &d,
                                        double &tot, double c, double s) {
    x += d * c;  // :135
    y += d * s;  // :136
    // v_fma_f64 with the constant from its SGPR pair (the compiler's v_fmac
    // form would first copy it into the accumulator, 2 v_movs per fma)
    double tx, ty;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tx) : "v"(x), "v"(L.ir), "s"(L.cxk));
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(ty) : "v"(y), "v"(L.ir), "s"(L.cyk));
    const uint32_t hx = dhi(tx), lx = dlo(tx), hy = dhi(ty), ly = dlo(ty);
    const uint32_t col = __builtin_amdgcn_alignbit(hx, lx, 30) - kFxU0;
    const uint32_t row = __builtin_amdgcn_alignbit(hy, ly, 30) - kFxU0;
    const bool inb = (col < L.W) & (row < L.H) & ((int32_t)hx >= 0x40000000) & ((int32_t)hy >= 0x40000000);
    const bool near = ((lx << 2) + 4u * kFxBand < 8u * kFxBand) | ((ly << 2) + 4u * kFxBand < 8u * kFxBand);
    const uint32_t fast = fx_offset(L.k1, row, col);
    const uint32_t sel = 0u - (uint32_t)inb;
    uint32_t off = (fast & sel) | (L.oobv & ~sel);
    if (__builtin_amdgcn_ballot_w64(near)) {  // wave-uniform, rare
        if (near) off = exact_offset(m, x, y, L.oobv);
    }
    d = fx_load(m.dt, off);
    tot += d;  // :141
}

// fx_step for a car whose rays cannot leave t's binade (SAFE: the scan
// origin lies within 2^21 - 16 cells of the map origin, less the max range;
// every lookup of a ray is within max_range of its origin, since the loop
// steps only while tot <= max_range): the sign / exponent tests drop out and
// the column and row are clamped into the padding, which holds dt[-1,-1].
__device__ __forceinline__ void fx_step_safe(const TiledMapView &m, const FxLoop &L, double &x, double &y, double &d,
                                             double &tot, double c, double s) {
    x += d * c;  // :135
    y += d * s;  // :136
    double tx, ty;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tx) : "v"(x), "v"(L.ir), "s"(L.cxk));
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(ty) : "v"(y), "v"(L.ir), "s"(L.cyk));
    const uint32_t lx = dlo(tx), ly = dlo(ty);
    const uint32_t col = __builtin_amdgcn_alignbit(dhi(tx), lx, 30) - kFxU0;
    const uint32_t row = __builtin_amdgcn_alignbit(dhi(ty), ly, 30) - kFxU0;
    const bool near = ((lx << 2) + 4u * kFxBand < 8u * kFxBand) | ((ly << 2) + 4u * kFxBand < 8u * kFxBand);
    uint32_t off = fx_offset(L.k1, min(row, L.H), min(col, L.W));
    if (__builtin_amdgcn_ballot_w64(near)) {  // wave-uniform, rare
        if (near) off = exact_offset(m, x, y, L.oobv);
    }
    d = fx_load(m.dt, off);
    tot += d;  // :141
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// The ray's outputs: clamp (:143-144), noise after the clamp
// (laser_models.py:450-452), check_ttc_jit's beam test on the noisy scan
// (laser_models.py:188-217), obs / scan entries (F110Env._pack_flat_obs);
// with other cars in the env (HANDOFF) the f64 range also goes to
// k_post_multi, whose agent ray_cast re-writes the entries it shortens.
template <bool HANDOFF>
__device__ __forceinline__ void fx_epilogue(const RayArgs &K, int g, int e, int b, double tot, double mr,
                                            double noise, double v) {
    const int64_t r = (int64_t)g * K.B + b;
    double range = tot > mr ? mr : tot;
    if (K.noise_ext || K.noise_std > 0.0) range += noise;
    if (v != 0.0 && ttc_may_fire_lane(range, K.side_max, v, K.ttc_thresh)) {  // (side, beam_cos) loaded only where TTC can fire
        const double bcos = K.beam_cos[b], side = K.side[b];
        if (ttc_fires(range, side, v * bcos, K.ttc_thresh)) K.ttc_hit[g] = 1;
    }
    if (K.obs && g == e * K.A) K.obs[(size_t)e * K.obs_len + b] = obs_scan_value(range, K.lidar_max);
    if (K.scans_f32) K.scans_f32[r] = (float)range;
    if (K.scans_f64) K.scans_f64[r] = range;
    if (HANDOFF) K.scan[r] = range;
}

// Diagnostic wave trace of the one-wave-block ray kernels (f110_debug_wave_trace;
// the pointer is null in every other launch): lane 0 stores the wave's start
// time (s_memrealtime, 100 MHz) at entry and its end time, hardware id, XCC and
// work item (item << 32 | car) at exit, 4 u64 per block, with vector stores.
__device__ __forceinline__ void wave_stamp_start(uint64_t *wt) {
    if (wt && threadIdx.x == 0) wt[4 * (size_t)blockIdx.x] = __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void wave_stamp_end(uint64_t *wt, uint32_t item, uint32_t g) {
    if (wt && threadIdx.x == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        uint64_t *o = wt + 4 * (size_t)blockIdx.x;
        o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = ((uint64_t)xcc << 32) | hw;
        o[3] = ((uint64_t)item << 32) | g;
    }
}
// the same per wave of a multi-wave block (k_rays_fxs): record w = the wave's work item
__device__ __forceinline__ void wave_stamp_start_w(uint64_t *wt, int w) {
    if (wt && (threadIdx.x & 63) == 0) wt[4 * (size_t)w] = __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void wave_stamp_end_w(uint64_t *wt, int w, uint32_t item, uint32_t g) {
    if (wt && (threadIdx.x & 63) == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        uint64_t *o = wt + 4 * (size_t)w;
        o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = ((uint64_t)xcc << 32) | hw;
        o[3] = ((uint64_t)item << 32) | g;
    }
}

// PAD (k_rays_fxn on the padded row-major table, kFxpBase; k_rays_fxs): the IEEE path of
// tiled_cell as a byte offset of the padded table; off-map reads go to cell
// (-P, -P), which holds dt[-1,-1] like every padding cell.
__device__ __forceinline__ uint32_t exact_offset_pad(const TiledMapView &m, double x, double y, uint32_t P) {
    const double xr = x - m.ox, yr = y - m.oy;
    const bool inb = (xr >= 0) & (xr < m.wres) & (yr >= 0) & (yr < m.hres);  // false for NaN
    if (!inb) return 0u;
    int32_t c = (int32_t)(xr / m.res);
    int32_t r = (int32_t)(yr / m.res);
    if (c >= m.W) {  // dt[r, W] is dt[r+1, 0] in the reference's row-major read
        c = 0;
        ++r;
    }
    return r >= m.H ? 0u : ((uint32_t)(r + (int32_t)P) * (uint32_t)m.wt + (uint32_t)(c + (int32_t)P)) * 8u;
}

// The obs entry's f32 division by lidar_max (k_rays_fxs): q = v * y,
// r = fma(-q, lm, v), q' = fma(r, y, q) with y = RN(1 / lm): q is within one
// ulp of v / lm, so q' is the correctly rounded quotient (Markstein's theorem)
// when no intermediate is subnormal; lanes with v < 2^-60 (and lidar_max
// outside [2^-30, 2^30], obs_rinv = 0) take the IEEE divide.  Checked
// exhaustively against the divide for every f32 v in [0, lm]
// (tests/test_obs_division.py).
__device__ __forceinline__ float obs_scan_value_fast(double r, float lmax, float rinv) {
    // obs_scan_value's NaN -> lmax, +inf -> lmax, -inf -> 0, clip: v_min_f32 returns its
    // other operand for a NaN, and -0.0 stays -0.0 (not < 0)
    float v = __builtin_fminf((float)r, lmax);
    v = v < 0.0f ? 0.0f : v;
    const float q = v * rinv;
    float q2 = __builtin_fmaf(__builtin_fmaf(-q, lmax, v), rinv, q);
    const bool ieee = !(v >= 0x1p-60f) | (rinv == 0.0f);
    if (__builtin_amdgcn_ballot_w64(ieee)) {  // rare (wave-uniform branch)
        asm volatile("" ::: "memory");  // the divide stays in the branch (not speculated and selected)
        if (ieee) q2 = v / lmax;
    }
    return q2;
}

template <class T>
__device__ __forceinline__ T ld_off(const T *base, uint32_t byte_off) {  // global_load v, v_off, s[base]
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}

}  // namespace f110
