// f110_batch.hip — the C-ABI building blocks outside the env step: k_scan_batch, k_dynamics,
// k_dynamics_ks and k_collision_* (f110_scan_batch, f110_dynamics_batch, f110_dynamics_ks_batch,
// f110_collision_batch, f110_collision_multiple).
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_beam_runs.h"
#include "f110_dynamics.h"
#include "f110_geometry.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_step_args.h"
#include "f110_step_device.h"
#include "f110_task_args.h"

namespace f110 {

// ------------------------------------------------------------------------
// ScanSimulator2D.scan with rng=None for M poses: one thread per ray, beam
// runs rebuilt per thread (cheap: < 20 runs), optional probes.
__global__ void __launch_bounds__(kBlock) k_scan_batch(ScanArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t n = 0;
    if (gid < a.M * a.B) {
        const int64_t m = gid / a.B;
        const int b = (int)(gid - m * a.B);
        const double *pose = a.poses + 3 * m;
        BeamRun runs[kMaxSeg];
        double t0 = first_theta_index(pose[2], a.fov, a.theta_dis);
        int nr = build_beam_runs(t0, a.inc, a.theta_dis, a.B, runs, kMaxSeg);
        double t = beam_theta_index(runs, nr, b);
        int ti = (int)t;
        if (ti >= a.theta_dis) ti = 0;
        double s = a.sines[ti], c = a.cosines[ti];
        double x = pose[0], y = pose[1];
        double d = a.map.dt[cell_index(a.map, x, y)];
        double tot = d;
        n = 1;
        while (d > a.eps && tot <= a.max_range) {
            x += d * c;
            y += d * s;
            d = a.map.dt[cell_index_fast(a.map, x, y)];
            tot += d;
            ++n;
        }
        if (tot > a.max_range) tot = a.max_range;
        a.scans[gid] = tot;
        if (a.lookups) a.lookups[gid] = (int32_t)n;
        if (a.hit_rc) {  // (r, c) of the last lookup; out-of-map reads report (-1, -1)
            double xt = x - a.map.ox, yt = y - a.map.oy;
            double xr = xt * a.map.oc + yt * a.map.os;
            double yr = -xt * a.map.os + yt * a.map.oc;
            int rr = -1, cc = -1;
            if (!(xr < 0 || xr >= a.map.wres || yr < 0 || yr >= a.map.hres || xr != xr || yr != yr)) {
                cc = (int)(xr / a.map.res);
                rr = (int)(yr / a.map.res);
            }
            a.hit_rc[2 * gid] = rr;
            a.hit_rc[2 * gid + 1] = cc;
        }
    }
    if (a.ctr) count_rays(a.ctr, n);
}

hipError_t launch_scan_batch(const ScanArgs &a, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    int64_t n = a.M * a.B;
    hipLaunchKernelGGL(k_scan_batch, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_dynamics(const double *__restrict__ x, const double *__restrict__ u,
                                                     double *__restrict__ f, int64_t M, f110_params p) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    double xs[7], fs[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) xs[k] = x[7 * i + k];
    vehicle_dynamics_st(xs, u[2 * i], u[2 * i + 1], p, fs);
#pragma unroll
    for (int k = 0; k < 7; ++k) f[7 * i + k] = fs[k];
}

hipError_t launch_dynamics_batch(const double *x, const double *u, double *f, int64_t M, const f110_params &p,
                                 hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dynamics, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, x, u, f, M, p);
    return hipGetLastError();
}

// vehicle_dynamics_ks over M kinematic states [M][5] (f110_dynamics_ks_batch).
__global__ void __launch_bounds__(kBlock) k_dynamics_ks(const double *__restrict__ x, const double *__restrict__ u,
                                                        double *__restrict__ f, int64_t M, f110_params p) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    double xs[5], fs[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) xs[k] = x[5 * i + k];
    vehicle_dynamics_ks(xs, u[2 * i], u[2 * i + 1], p, fs);
#pragma unroll
    for (int k = 0; k < 5; ++k) f[5 * i + k] = fs[k];
}

hipError_t launch_dynamics_ks_batch(const double *x, const double *u, double *f, int64_t M, const f110_params &p,
                                    hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dynamics_ks, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, x, u, f, M, p);
    return hipGetLastError();
}

// collision (collision_models.py:113-182, GJK) for M vertex pairs: one thread
// per pair, the pair's 2 x 8 doubles in registers (f110_collision_batch).
__global__ void __launch_bounds__(kBlock) k_collision_batch(const double *__restrict__ v1,
                                                            const double *__restrict__ v2, int64_t M,
                                                            uint8_t *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    double a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a[k] = v1[8 * i + k];
        b[k] = v2[8 * i + k];
    }
    out[i] = gjk_collision(a, b) ? 1 : 0;
}

hipError_t launch_collision_batch(const double *v1, const double *v2, int64_t M, uint8_t *out, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_collision_batch, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, v1, v2,
                       M, out);
    return hipGetLastError();
}

// collision_multiple (collision_models.py:184-212) for M independent sets of
// N bodies: one wave per set, its N(N-1)/2 pairs spread over the lanes, then
// lane 0 writes the flags and partner indices in the reference's (i, j)
// order, so the last colliding pair of each body wins as in the reference.
__global__ void __launch_bounds__(64) k_collision_multiple(const double *__restrict__ verts, int64_t M, int32_t N,
                                                           double *__restrict__ collisions, double *__restrict__ idx) {
    const int64_t m = blockIdx.x;
    if (m >= M) return;
    __shared__ uint8_t hit[kMaxMultiBodies * kMaxMultiBodies];
    const double *v = verts + (size_t)m * N * 8;
    const int P = N * (N - 1) / 2;
    for (int q = threadIdx.x; q < P; q += 64) {
        int i = 0, r = q;  // pair q -> (i, j), i < j, in the reference's loop order
        while (r >= N - 1 - i) {
            r -= N - 1 - i;
            ++i;
        }
        const int j = i + 1 + r;
        hit[i * N + j] = gjk_collision(v + 8 * i, v + 8 * j) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *c = collisions + (size_t)m * N, *ix = idx + (size_t)m * N;
    for (int i = 0; i < N; ++i) {
        c[i] = 0.0;
        ix[i] = -1.0;
    }
    for (int i = 0; i < N - 1; ++i)
        for (int j = i + 1; j < N; ++j)
            if (hit[i * N + j]) {
                c[i] = 1.0;
                c[j] = 1.0;
                ix[i] = (double)j;
                ix[j] = (double)i;
            }
}

hipError_t launch_collision_multiple(const double *verts, int64_t M, int32_t N, double *collisions, double *idx,
                                     hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_collision_multiple, dim3((unsigned)M), dim3(64), 0, s, verts, M, N, collisions, idx);
    return hipGetLastError();
}

}  // namespace f110
