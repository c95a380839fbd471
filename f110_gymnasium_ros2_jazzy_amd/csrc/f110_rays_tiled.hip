// f110_rays_tiled.hip — k_rays_tiled, the ray kernel of rotated maps (and the A/B family of
// axis-aligned ones): the EDT sphere-trace of ScanSimulator2D (trace_ray) on the 4x4-tiled table,
// scan noise, TTC test, obs / scan outputs.
#include <hip/hip_runtime.h>

#include "../../include/f110_debug.h"
#include "f110_beam_runs.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_rng.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

// One wave's rays of k_rays_tiled (a lane traces when `has`): beam index,
// trace_ray's loop (laser_models.py:106-146) with the given EDT lookup,
// clamp, noise, TTC flag, outputs.  The loop runs on wave-uniform control
// (while any lane is still tracing), so its counters live in SGPRs: no
// per-lane lookup counter in the loop body.
template <bool HANDOFF, class Lookup>
__device__ __forceinline__ WaveLookups trace_wave(const RayArgs &a, bool has, int g, int b, int e, int64_t r,
                                                  Lookup lookup) {
    const uint64_t hm = __builtin_amdgcn_ballot_w64(has);
    WaveLookups w{0u, (uint32_t)__popcll(hm), 0u};
    if (!hm) return w;
    const int B = a.B;
    double c = 0.0, s = 0.0, x = 0.0, y = 0.0, d = 0.0, v = 0.0, noise = 0.0;
    if (has) {
        double t = beam_theta_index(a.runs + (size_t)g * kMaxSeg, a.nruns[g], b);
        int ti = (int)t;  // int(theta_index), laser_models.py:124
        if (ti >= a.theta_dis) ti = 0;
        c = a.cosines[ti];
        s = a.sines[ti];
        x = a.ray0[g];
        y = a.ray0[a.EA + g];
        d = a.ray0[2 * a.EA + g];  // :129
        v = a.vel[g];
        // the ray's scan noise does not depend on the trace: drawn (or
        // loaded) here, it overlaps the set-up loads above
        const RayArgs &K = *kernarg_rays();
        if (K.noise_ext)
            noise = K.noise_ext[(size_t)e * B + b];
        else if (K.noise_std > 0.0)
            noise = K.noise_std * (double)beam_normal(K.seed, (uint64_t)(K.env_offset + e), K.noise_step[e], b);
    }
    double tot = d;  // :130 (lanes without a ray: d = 0, never traced)
    const double eps = a.eps, mr = a.max_range;
    uint32_t iters = 0, lane_iters = 0;
    for (;;) {
        const bool act = d > eps && tot <= mr;  // :133 (no loop-carried mask)
        // ballots of the bare compares are their lane masks (a ballot of the
        // conjunction would go through a VGPR)
        const uint64_t m = __builtin_amdgcn_ballot_w64(d > eps) & __builtin_amdgcn_ballot_w64(tot <= mr);
        if (!m) break;
        ++iters;
        lane_iters += (uint32_t)__popcll(m);
        if (act) {
            x += d * c;  // :135
            y += d * s;  // :136
            d = lookup(x, y);
            tot += d;    // :141
        }
    }
    w.total = w.lanes + lane_iters;  // the first lookup of every ray came from k_agents
    w.max = 1u + iters;
    if (!has) return w;
    // Epilogue fields are read through the kernarg pointer HERE, after the
    // loop: argument loads would otherwise sit at kernel entry and stay live
    // in SGPRs across the loop.
    const RayArgs &K = *kernarg_rays();
    double range = tot > mr ? mr : tot;  // :143-144
    if (K.noise_ext || K.noise_std > 0.0) range += noise;  // noise after the clamp (see store_ray)
    // state[3] after update_pose; check_ttc_jit on the noisy scan, before the
    // agent ray_cast (base_classes.py:597-599)
    if (v != 0.0 && ttc_may_fire_lane(range, K.side_max, v, K.ttc_thresh)) {
        const double bcos = K.beam_cos[b], side = K.side[b];
        if (ttc_fires(range, side, v * bcos, K.ttc_thresh)) K.ttc_hit[g] = 1;
    }
    // outputs straight from the ray; with other cars in the env (HANDOFF)
    // k_post_multi patches the beams its ray_cast shortens
    if (K.obs && g == e * a.A) K.obs[(size_t)e * K.obs_len + b] = obs_scan_value(range, K.lidar_max);
    if (K.scans_f32) K.scans_f32[r] = (float)range;
    if (K.scans_f64) K.scans_f64[r] = range;
    if (HANDOFF) K.scan[r] = range;
    return w;
}

// ------------------------------------------------------------------------
// k_rays_tiled: one thread per ray on the 4x4-tiled EDT, with the rotation
// compiled out for axis-aligned maps.  Same results as k_rays, bit for bit.
//
// One ray per lane, 8 waves per SIMD, no lane refill: the hardware wave
// scheduler absorbs the ragged ray lengths.  Measured alternatives that lost
// (DESIGN.md §3): 2 and 4 interleaved rays per lane (1.4x / 2x slower), a
// per-wave ray pool with lane refill (1.35x slower).
//
// Every ray also runs its TTC test (check_ttc_jit, laser_models.py:188-217,
// on the noisy pre-ray_cast scan) and raises its car's flag, and writes its
// observation / scan output entries.  Single-agent envs are then finished
// (k_post_single resolves the per-env state; no f64 scan hand-off at all).
// With other cars in the env (HANDOFF) the f64 range also goes to
// k_post_multi, whose agent ray_cast re-writes the entries it shortens.
//
// CH (chunked dispatch): a wave traces 64 consecutive beams of ONE car (beam
// chunk k of car g) instead of 64 consecutive rays of the flat ray index, and
// the grid walks the chunks in a_order (the forward-looking, long-ray chunks
// first), all cars of one chunk slot before the next.  Waves whose rays run
// longest start first and the short side-looking chunks fill in behind them,
// instead of a late long wave extending the tail of the launch.  With 4 cars
// per block and G4 = ceil(EA/4) blocks per slot, block -> XCD (block % 8)
// keeps all of a car's chunks on one XCD (and its L2) when G4 % 8 == 0.
//
// TRACE (diagnostic build only, f110_debug_wave_trace): lane 0 of every wave
// records its start / end time (s_memrealtime, 100 MHz), hardware id, XCC,
// chunk slot and car to a buffer nothing else reads.
template <bool ROT, bool MASK, bool HANDOFF, bool CH, bool TRACE = false>
__global__ void __launch_bounds__(kBlock) k_rays_tiled(RayArgs a) {
    uint64_t t_start = 0;
    if (TRACE) t_start = __builtin_amdgcn_s_memrealtime();
    const int B = a.B;
    int64_t r;
    int g, b;
    bool live;
    if (CH) {
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        int k;
        if ((int)blockIdx.x < a.HB) {  // heavy-first blocks: the listed waves
            const uint32_t item = (uint32_t)blockIdx.x * a.wpb + wave;
            if (item >= *a.heavy_count) return;  // wave-uniform: nothing listed here
            const uint32_t v = __builtin_amdgcn_readfirstlane(a.heavy_list[item]);
            g = (int)(v >> 8);
            k = (int)(v & 255u);
        } else {
            const int blk = (int)blockIdx.x - a.HB;
            const int slot = blk / a.G4;
            const int cg = blk - slot * a.G4;
            g = cg * a.wpb + wave;
            k = (int)a.order[slot];
            if (a.HB && g < a.EA && ((a.heavy_mask[g] >> k) & 1u)) return;  // ran in a heavy block
        }
        b = k * 64 + (int)(threadIdx.x & 63);
        live = g < a.EA && b < B;
        r = (int64_t)g * B + b;
    } else {
        r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        live = r < (int64_t)a.EA * B;
        g = (int)(r / B);
        b = (int)(r - (int64_t)g * B);
    }
    const int e = live ? g / a.A : 0;
    const bool has = live && (!MASK || a.reset_mask[e]);
    // the off-map cell index in a VGPR for the whole trace (an opaque copy:
    // otherwise it is re-materialised by a v_mov in every loop iteration)
    uint32_t oobv;
    asm volatile("v_mov_b32 %0, %1" : "=v"(oobv) : "s"((uint32_t)a.m.oob << 3));
    const WaveLookups w = trace_wave<HANDOFF>(a, has, g, b, e, r,
                                              [&](double x, double y) { return tiled_lookup<ROT>(a.m, x, y, oobv); });
    if ((threadIdx.x & 63) == 0 && w.lanes) {  // one (lookups, rays) atomic pair per wave
        unsigned long long *slot = kernarg_rays()->ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride;
        atomicAdd(slot, (unsigned long long)w.total);
        atomicAdd(slot + 1, (unsigned long long)w.lanes);
    }
    if (CH) {  // this wave's cost, the next step's heavy-first prediction
        const uint32_t m = w.lanes ? w.max : 0u;
        uint8_t *wc = kernarg_rays()->wcost;
        if (wc && (threadIdx.x & 63) == 0 && g < a.EA)
            wc[(size_t)g * a.nch + (b >> 6)] = (uint8_t)(m < 255u ? m : 255u);
    }
    if (TRACE && (threadIdx.x & 63) == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
        const int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
        uint64_t *o = kernarg_rays()->wtrace + 4 * w;
        o[0] = t_start;
        o[1] = t_end;
        o[2] = ((uint64_t)xcc << 32) | hw;
        o[3] = ((uint64_t)(CH ? (int)blockIdx.x / a.G4 : 0) << 32) | (uint32_t)g;
    }
}

// Every k_rays_tiled the library instantiates is named here: <ROT, MASK, HANDOFF, CH> for the flat
// and the chunked family; <.., TRACE>: the diagnostic wave trace.
RayKernel tiled_ray_kernel(const RayPlan &p) {
    static const RayKernel fn[2][8] = {
        {k_rays_tiled<false, false, false, false>, k_rays_tiled<false, false, true, false>,
         k_rays_tiled<false, true, false, false>, k_rays_tiled<false, true, true, false>,
         k_rays_tiled<true, false, false, false>, k_rays_tiled<true, false, true, false>,
         k_rays_tiled<true, true, false, false>, k_rays_tiled<true, true, true, false>},
        {k_rays_tiled<false, false, false, true>, k_rays_tiled<false, false, true, true>,
         k_rays_tiled<false, true, false, true>, k_rays_tiled<false, true, true, true>,
         k_rays_tiled<true, false, false, true>, k_rays_tiled<true, false, true, true>,
         k_rays_tiled<true, true, false, true>, k_rays_tiled<true, true, true, true>}};
    static const RayKernel trace[2] = {k_rays_tiled<false, false, false, true, true>,
                                       k_rays_tiled<false, false, true, true, true>};
    const int vt = (p.rot ? 4 : 0) + (p.mask ? 2 : 0) + (p.handoff ? 1 : 0);
    return p.trace ? trace[p.handoff] : fn[p.family == F110_RAY_TILED_CHUNKED][vt];
}

}  // namespace f110
