// f110_step_device.h — device code that more than one stage of the env step shares (f110_agents.hip,
// the f110_rays_*.hip files, f110_post.hip) and f110_batch.hip: wave reductions, the ray counters, the
// obs row and scan entry, the TTC beam test, the kernarg block's accessors and the (car, opponent)
// pair geometry.  Headers only: no stage's machine code depends on another stage's file.
#pragma once

#include <hip/hip_runtime.h>

#include "f110_beam_runs.h"
#include "f110_env_rows.h"
#include "f110_geometry.h"
#include "f110_sincos.h"
#include "f110_step_args.h"

namespace f110 {

constexpr int kBlock = kRayBlock;

static_assert(sizeof(BeamRun) == 24, "BeamRun layout");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One (lookups, rays) atomic pair per wave into a per-block slot.  n = lookups
// of this lane's rays (0 for a lane without rays), rays = rays per busy lane.
__device__ __forceinline__ void count_rays(unsigned long long *ctr, uint32_t n, uint32_t rays = 1) {
    uint32_t tot = wave_sum(n);
    uint32_t cnt = wave_sum(n ? rays : 0u);
    if ((threadIdx.x & 63) == 0 && cnt) {
        unsigned long long *slot = ctr + (size_t)(blockIdx.x % kCtrSlots) * kCtrStride;
        atomicAdd(slot, (unsigned long long)tot);
        atomicAdd(slot + 1, (unsigned long long)cnt);
    }
}

// floats between obs rows: f110_outputs.obs_stride, or packed B + 4A
__host__ __device__ __forceinline__ int64_t obs_row(const StepArgs &a) {
    return a.out.obs_stride ? a.out.obs_stride : (int64_t)a.B + 4 * a.A;
}

// F110Env._pack_flat_obs's scan entry (f110_env.py:557-560): f32, NaN ->
// lidar_max, +-inf -> lidar_max / 0, clip, / lidar_max in f32 (the f32 part: f110_env_rows.h).
__device__ __forceinline__ float obs_scan_value(double r, float lmax) { return obs_scan_value((float)r, lmax); }

// check_ttc_jit's per-beam test (laser_models.py:188-217):
//   ttc = (range - side) / proj_vel;  hit = ttc < thresh && ttc >= 0.
// The f64 divide only runs for beams that can fire: with num = range - side
// > 0 and num >= fl(1.2 * thresh * |proj_vel|), |num / proj_vel| >= 1.2 *
// thresh * (1 - 2^-53) > thresh, so the reference's test is false whatever
// the quotient rounds to.  Every other beam takes the exact divide.
__device__ __forceinline__ bool ttc_fires(double range, double side, double proj_vel, double thresh) {
    const double num = range - side;
    if (num > 0.0 && num >= (1.2 * thresh) * fabs(proj_vel)) return false;
    const double ttc = num / proj_vel;
    return ttc < thresh && ttc >= 0.0;
}

// ttc_fires' first test passed for EVERY beam of the car: with side <= side_max
// and |v beam_cos| <= |v| (rounding is monotonic), range - side_max > 0 and
// >= (1.2 thresh) |v| make it return false whatever the beam.  The caller
// loads (side, beam_cos) only for the lanes (and waves) where this is true.
__device__ __forceinline__ bool ttc_may_fire_lane(double range, double side_max, double v, double thresh) {
    const double nm = range - side_max;
    return !(nm > 0.0 && nm >= (1.2 * thresh) * fabs(v));
}

// The next step's heavy list starts empty (its counter is the other parity; k_agents fills this
// step's, build_heavy_list).
__device__ __forceinline__ void reset_next_heavy(const StepArgs &a) {
    if (a.heavy_count && blockIdx.x == 0 && threadIdx.x == 0) a.heavy_count[a.parity ^ 1] = 0;
}

// The RayArgs block in the kernarg segment (a ray kernel's only argument).
__device__ __forceinline__ const RayArgs *kernarg_rays() {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const RayArgs *>(__builtin_amdgcn_kernarg_segment_ptr());
#else
    return nullptr;
#endif
}

// The kernarg block behind an opaque copy of its pointer: loads through it
// stay where they are written (in the refill pass) instead of being hoisted
// out of the trace loop into SGPRs, which would spill there.  The copy is an
// SGPR pair typed in the constant address space: its field loads are scalar
// loads placed at the use (a generic pointer out of the asm would make them
// flat vector loads)
template <class T>
__device__ __forceinline__ const T *launder_const(const T *ptr) {
    const __attribute__((address_space(4))) T *p;
    asm volatile("s_mov_b64 %0, %1" : "=s"(p) : "s"(ptr));
    return (const T *)p;
}

__device__ __forceinline__ const RayArgs &kernarg_here() { return *launder_const(kernarg_rays()); }

// Lookup statistics of one wave's trace, the same in every lane: lookups
// made, lanes that traced a ray, the longest ray's lookups.
struct WaveLookups {
    uint32_t total, lanes, max;
};

// One (car i, opponent j) pair's ray_cast geometry, serially on one lane: the
// same functions and operands as k_post_multi's lane-parallel phases, so the
// same bits.  (xi, yi, yawi): car i's state pose (after the TTC response);
// (xj, yj, thj): opponent j's agent pose (before it, base_classes.py:587).
__device__ __forceinline__ void pair_geometry(double xi, double yi, double yawi, double xj, double yj, double thj,
                                              double length_i, double width_i, int B, double fov, double incr,
                                              double *rv, double *phi, double &wc, double &wh, int32_t *rng) {
    // rv / phi point into the result's own memory (global or LDS): box_beam_window indexes them
    // with loop variables, which local arrays would turn into scratch
    get_vertices(xj, yj, thj, length_i, width_i, rv);  // RaceCar i's params
    double ys, yc;
    cr_sincos(yawi, ys, yc);
    const double ego = atan2(ys, yc);
    int lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = blocked_vertex_beam(xi, yi, ego, rv[2 * q], rv[2 * q + 1], B, fov, incr, phi[q]);
        lo = (q == 0 || k < lo) ? k : lo;
        hi = (q == 0 || k > hi) ? k : hi;
    }
    double c, h;
    box_beam_window(xi, yi, rv, phi, c, h);
    int r0a, r0b, r1a, r1b;
    window_beam_ranges(yawi, fov, incr, B, c, h, r0a, r0b, r1a, r1b);
    wc = c;
    wh = h;
    rng[0] = r0a > lo ? r0a : lo;
    rng[1] = r0b < hi ? r0b : hi;
    rng[2] = r1a > lo ? r1a : lo;
    rng[3] = r1b < hi ? r1b : hi;
}

// pair_geometry out of line (k_post_multi's rare recompute after a TTC response):
// inlined, its transcendentals' constants were hoisted out of the block's loops
// and spilled
__device__ __noinline__ inline void pair_geometry_ool(double xi, double yi, double yawi, double xj, double yj,
                                                      double thj, double length_i, double width_i, int B, double fov,
                                                      double incr, double *rv, double *phi, double *wc, double *wh,
                                                      int32_t *rng) {
    pair_geometry(xi, yi, yawi, xj, yj, thj, length_i, width_i, B, fov, incr, rv, phi, *wc, *wh, rng);
}

}  // namespace f110
