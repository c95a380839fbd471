// f110_rays_fx.hip — k_rays_fx and k_rays_fxn: the chunked ray kernels with a fixed-point cell
// index (f110_rays_fx.h) on one-wave blocks, for masked resets and A/B on axis-aligned maps.
#include <hip/hip_runtime.h>

#include "../../include/f110_debug.h"
#include "f110_beam_runs.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_rays_fx.h"
#include "f110_rng.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

// ------------------------------------------------------------------------
// k_rays_fx: the chunked ray kernel with a fixed-point cell index (one-wave
// blocks, axis-aligned maps; same results as k_rays_tiled, bit for bit).
//
// Every lane runs one ray; lanes whose ray has ended leave the loop (exec
// mask), each lane counts its own lookups (summed once per wave), and cars
// whose rays stay in t's binade take fx_step_safe (~36 instead of ~59
// instructions per iteration on the wave's serial path; the kernel is
// latency-bound: at 6 / 4 / 2 waves per SIMD it takes 1.31x / 1.62x / 2.9x as
// long).  Row-major EDT with dt[-1,-1] in the padding.
template <bool MASK, bool HANDOFF>
__global__ void __launch_bounds__(64) k_rays_fx(RayArgs a) {
    int g, k;
    if ((int)blockIdx.x < a.HB) {  // heavy-first blocks: the listed waves
        const uint32_t item = blockIdx.x;
        if (item >= ld_const(a.heavy_count)) return;
        const uint32_t v = ld_const(a.heavy_list + item);
        g = (int)(v >> 8);
        k = (int)(v & 255u);
    } else {
        const int blk = (int)blockIdx.x - a.HB;
        const int slot = blk / a.G4;
        g = blk - slot * a.G4;
        k = (int)a.order[slot];
        if (g >= a.EA) return;
        if (a.HB && ((ld_const(a.heavy_mask + g) >> k) & 1u)) return;  // ran in a heavy block
    }
    wave_stamp_start(a.wtrace);
    const int lane = (int)threadIdx.x;
    const int B = a.B;
    const int b0 = k * 64;
    const int b = b0 + lane;
    const int e = HANDOFF ? g / a.A : g;
    const bool has = b < B && (!MASK || ld_const(a.reset_mask + e));

    // ---- per-car set-up (wave-uniform: scalar loads) ----
    // get_scan's beam index (laser_models.py:167-184) from the car's runs:
    // the run holding b0 by a scalar binary search, then the (few) runs that
    // start inside this wave's 64 beams
    const BeamRun *R = a.runs + (size_t)g * kMaxSeg;
    const int n = ld_const(a.nruns + g);
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ld_const(&R[mid].start) <= b0) lo = mid;
        else hi = mid - 1;
    }
    int rs = ld_const(&R[lo].start);
    double t0 = ld_const(&R[lo].t0), dl = ld_const(&R[lo].delta);
    for (int j = lo + 1; j < n; ++j) {
        const int s2 = ld_const(&R[j].start);
        if (s2 > b0 + 63) break;
        if (b >= s2) {
            rs = s2;
            t0 = ld_const(&R[j].t0);
            dl = ld_const(&R[j].delta);
        }
    }
    const double x00 = ld_const(a.ray0 + g), y00 = ld_const(a.ray0 + a.EA + g);
    const double d00 = ld_const(a.ray0 + 2 * a.EA + g);  // :129
    const double v = ld_const(a.vel + g);
    // every lane runs the set-up (lanes past the last beam on beam B-1, their
    // results unused): no divergent branch, no zero-initialised copies
    const int bc = b < B ? b : B - 1;
    const double t = t0 + (double)(bc - rs) * dl;
    int ti = (int)t;  // int(theta_index), laser_models.py:124
    if (ti >= a.theta_dis) ti = 0;
    const double c = a.cosines[ti], s = a.sines[ti];
    double x = x00, y = y00, d = has ? d00 : 0.0;
    double noise = 0.0;
    {
        const RayArgs &K = *kernarg_rays();
        if (K.noise_ext)
            noise = K.noise_ext[(size_t)e * B + bc];
        else if (K.noise_std > 0.0)
            noise = K.noise_std *
                    (double)beam_normal_k(noise_key(K.seed, (uint64_t)(K.env_offset + e)), ld_const(K.noise_step + e), bc);
    }

    // ---- trace_ray's loop (laser_models.py:133-141) ----
    const FxLoop L = fx_loop(a);
    double tot = d;  // :130 (lanes without a ray: d = 0, never traced)
    uint32_t cnt = 0;
    const double qx = fma(x00, L.ir, L.cxk) - kFxMagic, qy = fma(y00, L.ir, L.cyk) - kFxMagic;
    __builtin_amdgcn_s_waitcnt(0);  // the set-up loads (c, s) land before the loop, not in it
    if (fabs(qx) < a.fx_lim && fabs(qy) < a.fx_lim) {  // wave-uniform (false for NaN)
        while ((dhi(d) != 0u) & (tot <= L.mr)) {
            fx_step_safe(a.m, L, x, y, d, tot, c, s);
            ++cnt;
        }
    } else {
        while ((dhi(d) != 0u) & (tot <= L.mr)) {
            fx_step(a.m, L, x, y, d, tot, c, s);
            ++cnt;
        }
    }
    const uint32_t lane_iters = wave_sum(cnt);
    // the wave's trip count (heavy-first cost; lane slots of the SIMT counter)
    const uint32_t iters = (a.wcost || a.count_slots) ? wave_max(cnt) : 0u;

    // ---- epilogue ----
    const uint32_t lanes = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(has));
    if (has) fx_epilogue<HANDOFF>(*kernarg_rays(), g, e, b, tot, L.mr, noise, v);
    if (lane == 0) {
        const RayArgs &K = *kernarg_rays();
        if (lanes) {  // one (lookups, rays) atomic pair per wave; the first lookup came from k_agents
            unsigned long long *slot = K.ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride;
            atomicAdd(slot, (unsigned long long)(lanes + lane_iters));
            atomicAdd(slot + 1, (unsigned long long)lanes);
            if (K.count_slots) atomicAdd(slot + 2, (unsigned long long)iters * 64ull);  // lane slots the loop issued
        }
        if (K.wcost) {  // this wave's cost, the next step's heavy-first prediction
            const uint32_t mx = lanes ? 1u + iters : 0u;
            K.wcost[(size_t)g * a.nch + k] = (uint8_t)(mx < 255u ? mx : 255u);
        }
    }
    wave_stamp_end(kernarg_here().wtrace, (uint32_t)k, (uint32_t)g);
}


// One fixed-point step of ray r of an ILP lane (k_rays_fxn, row-major table):
// the cell's byte offset for an active ray, the zero cell's (a 0.0 past the
// table's end, which no clamped index reaches) for a ray that has ended, so
// that its load returns d = 0 and leaves its total, x and y as they are.
__device__ __forceinline__ uint32_t fxn_offset(const TiledMapView &m, const FxLoop &L, double &x, double &y,
                                               double d, double c, double s, bool act, uint64_t amask,
                                               uint32_t zero) {
    x += d * c;  // :135
    y += d * s;  // :136
    double tx, ty;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tx) : "v"(x), "v"(L.ir), "s"(L.cxk));
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(ty) : "v"(y), "v"(L.ir), "s"(L.cyk));
    const uint32_t lx = dlo(tx), ly = dlo(ty);
    const uint32_t col = __builtin_amdgcn_alignbit(dhi(tx), lx, 30) - kFxU0;
    const uint32_t row = __builtin_amdgcn_alignbit(dhi(ty), ly, 30) - kFxU0;
    // ballots of bare compares are their lane masks; a ballot of a combined
    // bool would first be materialised in a VGPR (2 more VALU per ballot)
    const uint32_t band = min((lx << 2) + 4u * kFxBand, (ly << 2) + 4u * kFxBand);
    uint32_t fast = fx_offset(L.k1, min(row, L.H), min(col, L.W));
    asm volatile("" : "+v"(fast));  // computed for every lane, then selected (no exec-mask branch)
    uint32_t off = act ? fast : zero;
    if (__builtin_amdgcn_ballot_w64(band < 8u * kFxBand) & amask) {  // wave-uniform, rare
        if (act & (band < 8u * kFxBand)) off = exact_offset(m, x, y, L.oobv);
    }
    return off;
}

// One step of ray r of a PAD lane whose car passed the origin test (every
// lookup of its rays lies inside the padded table, fxp_lo / fxp_hx / fxp_hy):
// t = fma(x, inv_res, 2^24 + P - origin / res); one v_alignbit by 28 puts
// floor(q) + P in the low 24 bits, which the u24 multiplies read directly --
// no bias subtraction, no bounds test, no clamp (~15 instead of ~20 VALU per
// ray and iteration in fxn_offset).  Ended rays read the zero cell, lanes
// within kFxpBand * 2^-28 of a cell edge take the IEEE path.
__device__ __forceinline__ uint32_t fxp_offset(const TiledMapView &m, const FxLoop &L, double &x, double &y,
                                               double d, double c, double s, bool act, uint64_t amask,
                                               uint32_t zero_v, uint32_t P) {
    x += d * c;  // :135
    y += d * s;  // :136
    double tx, ty;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tx) : "v"(x), "v"(L.ir), "s"(L.cxk));
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(ty) : "v"(y), "v"(L.ir), "s"(L.cyk));
    const uint32_t lx = dlo(tx), ly = dlo(ty);
    const uint32_t col = __builtin_amdgcn_alignbit(dhi(tx), lx, 28);
    const uint32_t row = __builtin_amdgcn_alignbit(dhi(ty), ly, 28);
    const uint32_t band = min((lx << 4) + 16u * kFxpBand, (ly << 4) + 16u * kFxpBand);
    // (row & 0xffffff) * k1 + (col & 0xffffff) * 8: v_mul_u32_u24 + v_mad_u32_u24 (the compiler's
    // form of the second multiply is a shift and a mask, one more VALU)
    const uint32_t prow = __umul24(row, L.k1);
    uint32_t fast;
    asm volatile("v_mad_u32_u24 %0, %1, 8, %2" : "=v"(fast) : "v"(col), "v"(prow));
    uint32_t off = act ? fast : zero_v;
    if (__builtin_amdgcn_ballot_w64(band < 32u * kFxpBand) & amask) {  // wave-uniform, rare
        if (act & (band < 32u * kFxpBand)) off = exact_offset_pad(m, x, y, P);
    }
    return off;
}

// k_rays_fxn: N rays per lane (beams b0 + 64 r + lane, r < N, of one car: N
// adjacent 64-beam chunks), traced in one loop so that each lane keeps N
// independent EDT gathers in flight.  The single-ray kernel is bound by the
// latency of its dependent gather chain, not by issue (at 6 / 4
// / 2 waves per SIMD it takes 1.31x / 1.62x / 2.9x as long).  A ray that has
// ended reads the zero cell (d = 0); a chunk whose rays have all ended skips
// its step (wave-uniform); the active-ray masks are ballots, so the lookup
// count is a scalar popcount.  Cars whose rays could leave t's binade trace
// their N rays one after the other with fx_step.  Row-major EDT with
// dt[-1,-1] in the padding column / row.  Bit-identical to k_rays_fx.
//
// Heavy-first (as k_rays_fx, with a chunk group in place of a chunk: a.nch is
// the number of groups per car here): HB leading blocks run the groups whose
// longest ray took >= heavy_T lookups in the previous launch.
template <int N, bool MASK, bool HANDOFF, bool PAD = false>
__global__ void __launch_bounds__(64, 8) k_rays_fxn(RayArgs a) {  // 8 waves per SIMD: <= 64 VGPRs
    const int ng = a.nch;  // chunk groups of N chunks per car
    int g, grp;
    if ((int)blockIdx.x < a.HB) {  // heavy-first blocks: the listed groups
        const uint32_t item = blockIdx.x;
        if (item >= ld_const(a.heavy_count)) return;
        const uint32_t hv = ld_const(a.heavy_list + item);
        g = (int)(hv >> 8);
        grp = (int)(hv & 255u);
    } else {
        const int blk = (int)blockIdx.x - a.HB;
        const int slot = blk / a.G4;
        g = blk - slot * a.G4;
        if (g >= a.EA) return;
        grp = ng - 1 - slot;  // descending, as the chunk order of k_rays_fx
        if (a.HB && ((ld_const(a.heavy_mask + g) >> grp) & 1u)) return;  // ran in a heavy block
    }
    wave_stamp_start(a.wtrace);
    const int lane = (int)threadIdx.x;
    const int B = a.B;
    const int b0 = grp * 64 * N;
    const int e = HANDOFF ? g / a.A : g;
    const bool live = !MASK || ld_const(a.reset_mask + e);

    // ---- per-car set-up (wave-uniform: scalar loads), as in k_rays_fx ----
    const BeamRun *R = a.runs + (size_t)g * kMaxSeg;
    const int n = ld_const(a.nruns + g);
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ld_const(&R[mid].start) <= b0) lo = mid;
        else hi = mid - 1;
    }
    int rs[N];
    double t0[N], dl[N];
    {
        const int s0 = ld_const(&R[lo].start);
        const double u0 = ld_const(&R[lo].t0), w0 = ld_const(&R[lo].delta);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            rs[r] = s0;
            t0[r] = u0;
            dl[r] = w0;
        }
    }
    for (int j = lo + 1; j < n; ++j) {
        const int s2 = ld_const(&R[j].start);
        if (s2 > b0 + 64 * N - 1) break;
        const double tj = ld_const(&R[j].t0), dj = ld_const(&R[j].delta);
#pragma unroll
        for (int r = 0; r < N; ++r)
            if (b0 + 64 * r + lane >= s2) {
                rs[r] = s2;
                t0[r] = tj;
                dl[r] = dj;
            }
    }
    const double x00 = ld_const(a.ray0 + g), y00 = ld_const(a.ray0 + a.EA + g);
    const double d00 = ld_const(a.ray0 + 2 * a.EA + g);  // :129
    double x[N], y[N], d[N], tot[N], c[N], sn[N];
    int bc[N];
    bool has[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        const int b = b0 + 64 * r + lane;
        has[r] = live && b < B;
        bc[r] = b < B ? b : B - 1;
        int ti = (int)(t0[r] + (double)(bc[r] - rs[r]) * dl[r]);  // int(theta_index), :124
        if (ti >= a.theta_dis) ti = 0;
        c[r] = a.cosines[ti];
        sn[r] = a.sines[ti];
        x[r] = x00;
        y[r] = y00;
        d[r] = has[r] ? d00 : 0.0;
        tot[r] = d[r];  // :130
    }

    // ---- trace_ray's loop (laser_models.py:133-141), N rays per lane ----
    const FxLoop L = fx_loop(a);
    const uint32_t zero = a.fx_zero;
    uint32_t zero_v;  // in a VGPR for the whole trace (the select's other operand is its SGPR mask)
    asm volatile("v_mov_b32 %0, %1" : "=v"(zero_v) : "s"(zero));
    const uint32_t P = (uint32_t)a.fxp_P;
    uint32_t lane_iters = 0, iters = 0;
    bool fast_car;
    if (PAD) {  // q + P of the scan origin inside [fxp_lo, fxp_h*): its rays stay in the padded table
        const double ux = fma(x00, L.ir, L.cxk) - kFxpBase, uy = fma(y00, L.ir, L.cyk) - kFxpBase;
        fast_car = (ux >= a.fxp_lo) & (ux < a.fxp_hx) & (uy >= a.fxp_lo) & (uy < a.fxp_hy);  // false for NaN
    } else {
        const double qx = fma(x00, L.ir, L.cxk) - kFxMagic, qy = fma(y00, L.ir, L.cyk) - kFxMagic;
        fast_car = fabs(qx) < a.fx_lim && fabs(qy) < a.fx_lim;
    }
    __builtin_amdgcn_s_waitcnt(0);  // the set-up loads land before the loop, not in it
    if (fast_car) {  // wave-uniform (false for NaN)
        // no per-ray flag is carried across iterations (an i1 array would be
        // packed into a VGPR): activity is recomputed from d and the total
        for (;;) {
            uint64_t m[N], any = 0;
#pragma unroll
            for (int r = 0; r < N; ++r) {
                m[r] = __builtin_amdgcn_ballot_w64(dhi(d[r]) != 0u) & __builtin_amdgcn_ballot_w64(tot[r] <= L.mr);
                any |= m[r];
                lane_iters += (uint32_t)__popcll(m[r]);
            }
            if (!any) break;
            ++iters;
            uint32_t off[N];
#pragma unroll
            for (int r = 0; r < N; ++r) {
                off[r] = zero;
                if (m[r]) {
                    const bool act = (dhi(d[r]) != 0u) & (tot[r] <= L.mr);
                    off[r] = PAD ? fxp_offset(a.m, L, x[r], y[r], d[r], c[r], sn[r], act, m[r], zero_v, P)
                                 : fxn_offset(a.m, L, x[r], y[r], d[r], c[r], sn[r], act, m[r], zero);
                }
            }
#pragma unroll
            for (int r = 0; r < N; ++r) d[r] = fx_load(a.m.dt, off[r]);
#pragma unroll
            for (int r = 0; r < N; ++r) tot[r] += d[r];  // :141
        }
    } else {
        uint32_t cnt = 0;
#pragma unroll
        for (int r = 0; r < N; ++r)
            while ((dhi(d[r]) != 0u) & (tot[r] <= L.mr)) {
                if (PAD) {  // a car whose origin is off the map: the IEEE cell of every lookup
                    x[r] += d[r] * c[r];  // :135
                    y[r] += d[r] * sn[r];  // :136
                    d[r] = fx_load(a.m.dt, exact_offset_pad(a.m, x[r], y[r], P));
                    tot[r] += d[r];  // :141
                } else {
                    fx_step(a.m, L, x[r], y[r], d[r], tot[r], c[r], sn[r]);
                }
                ++cnt;
            }
        lane_iters = wave_sum(cnt);
        iters = wave_max(cnt);
    }

    // ---- epilogue ----
    const RayArgs &K = *kernarg_rays();
    const double v = ld_const(a.vel + g);
    uint32_t lanes = 0;
    const bool noise_on = K.noise_ext || K.noise_std > 0.0;
    const uint32_t key = noise_key(K.seed, (uint64_t)(K.env_offset + e));
    const uint64_t step = noise_on && !K.noise_ext ? ld_const(K.noise_step + e) : 0;
    float pn[N];  // device-stream normals: with N = 2 the lane's beams b and b + 64 share one draw
    if (!K.noise_ext && K.noise_std > 0.0) {
        if (N == 2) {
            beam_normal_pair_k(key, step, beam_noise_pair(b0 + lane), pn[0], pn[1]);
        } else {
#pragma unroll
            for (int r = 0; r < N; ++r) pn[r] = beam_normal_k(key, step, bc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double nz = 0.0;
        if (K.noise_ext) nz = K.noise_ext[(size_t)e * B + bc[r]];
        else if (K.noise_std > 0.0) nz = K.noise_std * (double)pn[r];
        if (has[r])
            fx_epilogue<HANDOFF>(K, g, e, b0 + 64 * r + lane, tot[r], L.mr, nz, v);
        lanes += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(has[r]));
    }
    if (lane == 0) {
        if (lanes) {  // one (lookups, rays) atomic pair per wave; the first lookup came from k_agents
            unsigned long long *cs = K.ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride;
            atomicAdd(cs, (unsigned long long)(lanes + lane_iters));
            atomicAdd(cs + 1, (unsigned long long)lanes);
            // lane slots the loop issued: trip count x 64 lanes x N rays (the serial
            // IEEE loop of an off-map car counts its longest lane's total, a lower bound)
            if (K.count_slots) atomicAdd(cs + 2, (unsigned long long)iters * (fast_car ? 64ull * N : 64ull));
        }
        if (K.wcost) {  // this group's cost, the next step's heavy-first prediction
            const uint32_t mx = lanes ? 1u + iters : 0u;
            K.wcost[(size_t)g * ng + grp] = (uint8_t)(mx < 255u ? mx : 255u);
        }
    }
    wave_stamp_end(kernarg_here().wtrace, (uint32_t)grp, (uint32_t)g);
}

// Every k_rays_fx / k_rays_fxn the library instantiates is named here: k_rays_fx<MASK, HANDOFF>,
// k_rays_fxn<2, MASK, HANDOFF, PAD> on the clamped and on the padded table.
RayKernel fx_ray_kernel(const RayPlan &p) {
    static const RayKernel fn[3][4] = {
        {k_rays_fx<false, false>, k_rays_fx<false, true>, k_rays_fx<true, false>, k_rays_fx<true, true>},
        {k_rays_fxn<2, false, false>, k_rays_fxn<2, false, true>, k_rays_fxn<2, true, false>,
         k_rays_fxn<2, true, true>},
        {k_rays_fxn<2, false, false, true>, k_rays_fxn<2, false, true, true>, k_rays_fxn<2, true, false, true>,
         k_rays_fxn<2, true, true, true>}};
    return fn[p.family - F110_RAY_FX][(p.mask ? 2 : 0) + (p.handoff ? 1 : 0)];
}

}  // namespace f110
