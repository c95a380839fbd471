// f110_step.cpp — one f110_step / f110_reset = three launches on the caller's stream:
//
//  k_agents    (f110_agents.hip) one thread per car: reset/autoreset, RaceCar.update_pose, scan
//              pose, first EDT lookup, and the car's beam-index runs.
//  k_rays_*    the lidar rays: the EDT sphere-trace of ScanSimulator2D (trace_ray), scan noise, TTC
//              test, obs / scan outputs.  k_rays_fxs (f110_rays_fxs.hip), k_rays_fx / k_rays_fxn
//              (f110_rays_fx.hip) on axis-aligned maps (fixed-point cell index), k_rays_tiled
//              (f110_rays_tiled.hip) on rotated ones; plan_ray_launch (f110_host.cpp) chooses.
//  k_post_*    (f110_post.hip) TTC response, obs packing, _check_done.
//
// No kernel lives here: each stage's file exports its launcher or its table of instantiations
// (f110_step_args.h).  Measured-slower variants live in git history and DESIGN.md, not here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>

#include "../../include/f110_debug.h"
#include "f110_map.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

// The kernel of a plan, from its family's table.
static RayKernel ray_kernel_fn(const RayPlan &p) {
    switch (p.family) {
    case F110_RAY_TILED_FLAT:
    case F110_RAY_TILED_CHUNKED:
        return tiled_ray_kernel(p);
    case F110_RAY_FX:
    case F110_RAY_FXN_CLAMPED:
    case F110_RAY_FXN_PADDED:
        return fx_ray_kernel(p);
    case F110_RAY_FXS:
        return fxs_ray_kernel(p);
    }
    return nullptr;
}

// The ray kernel's argument block for plan p.
static RayArgs ray_args(const StepArgs &a, const RayLaunch &r, const RayPlan &p) {
    const int EA = a.E * a.A;
    RayArgs ra{};
    ra.reset_mask = a.mode == 1 ? a.reset_mask : nullptr;
    // the common fields
    ra.m = a.tmap;
    ra.sines = a.sines;
    ra.cosines = a.cosines;
    ra.ray0 = a.ray0;
    ra.runs = a.runs;
    ra.nruns = a.nruns;
    ra.scan = a.scan;
    ra.noise_ext = a.noise_ext;
    ra.noise_step = a.noise_step;
    ra.ctr = a.ctr;
    ra.count_slots = r.k.count_slots;
    ra.eps = a.eps;
    ra.max_range = a.max_range;
    ra.noise_std = a.noise_std;
    ra.seed = a.seed;
    ra.env_offset = a.env_offset;
    ra.EA = EA;
    ra.A = a.A;
    ra.B = a.B;
    ra.theta_dis = a.theta_dis;
    ra.vel = a.st + (size_t)3 * EA;
    ra.beam_cos = a.beam_cos;
    ra.side = a.side;
    ra.cs2 = a.cs2;
    ra.bs2 = a.bs2;
    ra.ttc_thresh = a.ttc_thresh;
    ra.side_max = a.side_max;
    ra.ttc_hit = a.ttc_hit;
    ra.obs = a.out.obs;
    ra.obs_len = (int32_t)obs_row(a);
    ra.lidar_max = (float)a.p.lidar_max;
    ra.obs_rinv = obs_reciprocal(ra.lidar_max);
    ra.scans_f32 = a.out.scans;
    ra.scans_f64 = a.out.scans_f64;
    ra.wtrace = r.wtrace;
    ra.wpb = p.wpb;
    ra.G4 = p.G4;
    ra.nch = p.nch;
    ra.HB = p.HB;
    if (p.family != F110_RAY_TILED_FLAT) std::copy(r.chunk_order, r.chunk_order + kMaxChunks, ra.order);
    if (p.wcost) ra.wcost = a.wcost;
    if (p.HB) {  // this step's list of heavy waves
        ra.heavy_list = a.heavy_list + (size_t)a.parity * a.heavy_cap;
        ra.heavy_mask = a.heavy_mask;
        ra.heavy_count = a.heavy_count + a.parity;
    }
    // the EDT table (ra.m is the 4x4-tiled one so far) and the cell-index constants that go with it
    if (p.table != F110_TABLE_TILED) {
        const bool pad = p.table == F110_TABLE_PADDED;
        const FxTable &t = pad ? r.rmp : r.rm;
        const TiledMapView &tm = a.tmap;
        // clamped: t = x / res + 1.5 * 2^22 (kFxMagic); padded (PAD): t = x / res + 2^24 + P
        const double P = (double)t.P, base = pad ? kFxpBase + P : kFxMagic;
        ra.m.dt = t.dt;
        ra.m.wt = t.w;
        ra.m.oob = (int32_t)t.oob;
        ra.fx_zero = t.zero;
        ra.fxp_P = t.P;
        ra.fx_cx = std::fma(-tm.ox, tm.inv_res, base);
        ra.fx_cy = std::fma(-tm.oy, tm.inv_res, base);
        ra.fx_lim = 2097152.0 - 32.0 - a.max_range * tm.inv_res;
        if (pad) {
            // a car's rays stay in the padded table when its origin's q + P lies in [Rn, W or H + 2P - Rn),
            // Rn = max_range / res + 2 cells (each lookup is within max_range of it)
            const double Rn = std::ceil(a.max_range * tm.inv_res) + 2.0;
            ra.fxp_lo = Rn;
            ra.fxp_hx = (double)tm.W + 2.0 * P - Rn;
            ra.fxp_hy = (double)tm.H + 2.0 * P - Rn;
            ra.fxs_cx = std::fma(-tm.ox, tm.inv_res, kFxsBase + P + kFxsShift);
            ra.fxs_cy = std::fma(-tm.oy, tm.inv_res, kFxsBase + P + kFxsShift);
        }
    }
    if (p.geo_ready) {  // k_rays_fxs<HANDOFF>'s leading items compute the pairs' ray_cast geometry
        ra.geo = a.geo;
        ra.hmask = a.hmask;
        ra.geo_blocks = p.geo_blocks;
        ra.st = a.st;
        ra.pa = a.pa;
        ra.fov = a.fov;
        ra.beam_incr = a.beam_incr;
    }
    return ra;
}

// One f110_step / f110_reset: k_agents, the ray kernel plan_ray_launch chose, the post stage.
hipError_t launch_env_step(const StepArgs &a, const RayLaunch &r, hipStream_t s, hipEvent_t *ev) {
    hipError_t e;
    auto evk = [&](int i) -> hipEvent_t { return ev ? ev[i] : nullptr; };  // (start, stop) per kernel
    if ((e = launch_agents(a, s, evk(0), evk(1))) != hipSuccess) return e;
    if (r.gate_wait && (e = hipStreamWaitEvent(s, r.gate_wait, 0)) != hipSuccess) return e;
    // f110_debug_set_handoff_check: every hand-off entry NaN (all-ones) before the ray launch, so a
    // k_post_multi read of an entry the ray kernel skipped cannot pass for a fresh one
    if ((a.hcheck & 1) && a.A != 1 &&
        (e = hipMemsetAsync(a.scan, 0xFF, (size_t)a.E * a.A * a.B * sizeof(double), s)) != hipSuccess)
        return e;
    const RayPlan p = plan_ray_launch(r.k, a.mode == 1 && a.reset_mask != nullptr);
    RayArgs ra = ray_args(a, r, p);
    void *args[] = {&ra};
    if ((e = hipExtLaunchKernel(reinterpret_cast<const void *>(ray_kernel_fn(p)), dim3(p.grid), dim3(p.block), args, 0u,
                                s, evk(2), evk(3), 0)) != hipSuccess)
        return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (r.gate_record && (e = hipEventRecord(r.gate_record, s)) != hipSuccess) return e;
    return launch_post(a, p.geo_ready, s, evk(4), evk(5));
}

}  // namespace f110
