// f110_track_obs.hip — the track-relative observation block on the device (f110_track_obs /
// f110_ctx_track_obs, include/f110.h "track observation"): the seat car's dynamic state, its
// lateral offset and heading error on the centerline, a preview of the centerline ahead in the
// car's frame and the other car's gap, as float32 columns appended to each env's obs row.  No
// reference counterpart (_pack_flat_obs stops at the map poses); the projection is the reward's
// (f110_track_device.h), the row rule f110_track_obs.h's, which f110_host_track_obs states on the
// host.
//
//   k_track_obs  one wave per env, four envs per 256-thread block, as k_race_project: the seat's
//                point on lanes 0-31, the other car's on 32-63, through project_xy, so the two
//                dependent load chains (grid bounds -> midpoints -> segment ends) overlap and every
//                cross-lane step of the projection stays inside its half.  A half whose car is
//                missing or not finite skips the projection as a whole: no half is ever divided
//                around a shuffle.  Both halves then meet again and the seat half reads the other's
//                (s, t, v, ok) from lane 32 -- the one cross-half read -- after which the upper
//                half leaves.  Lane j < n_preview of the seat half resolves preview point j (seg_at
//                is a per-lane search from the projection's segment); the seat's own seven columns
//                and the gap's three are lane-uniform arithmetic.  Lane c < width then picks column
//                c (the preview's through one shuffle inside the half) and the row goes out as one
//                coalesced store.  Every column has one writer, the pad columns included (+0).
//
// No LDS, no barrier, no atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_sincos.h"
#include "f110_task_args.h"
#include "f110_track_device.h"
#include "f110_track_obs.h"

namespace f110 {

namespace {

static_assert(kTrackObsMaxWidth <= kHalf, "a row's columns are gathered inside the seat's half-wave");

__global__ void __launch_bounds__(64 * kRaceProjEnvs) k_track_obs(TrackObsArgs a) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (kHalf - 1);
    const int upper = lane >> 5;  // 0: the seat's half, 1: the other car's
    const int64_t e = (int64_t)blockIdx.x * kRaceProjEnvs + (threadIdx.x >> 6);
    if (e >= a.E) return;  // the whole wave
    const TrackView &T = a.track;
    const f110_track_obs_params &P = a.p;
    const int32_t car = upper ? a.other : a.seat;  // half-uniform
    TrackObsCar c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool ok = car >= 0;
    if (ok) {
        c = track_obs_car(a.state, a.E * a.A, e * a.A + car);
        ok = isfinite(c.x) && isfinite(c.y) && (upper || isfinite(c.yaw));
    }
    Proj pj{0.0, 0.0, 0};
    if (ok) pj = project_xy(T, c.x, c.y, sub);  // all 32 lanes of the half, or none
    // the whole wave again: the other car's result to the seat's half
    const double s_o = __shfl(pj.s, kHalf, 64), t_o = __shfl(pj.t, kHalf, 64), v_o = __shfl(c.v, kHalf, 64);
    const int ok_o = __shfl((int)ok, kHalf, 64);
    if (upper) return;
    const int np = P.n_preview;
    double val = 0.0;  // a row that is not ok, and the pad columns: +0
    if (ok) {          // half-uniform
        double sn, cs;
        cr_sincos(c.yaw, sn, cs);
        double px = 0.0, py = 0.0;
        if (sub < np) {  // preview point `sub`
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < kTrackObsMaxPreview; ++j)  // (a select chain: no indexed copy of the params)
                if (sub == j) d = P.preview[j];
            const double sq = track_obs_query(P, d, pj.s, T.closed, T.L);
            const int32_t k = seg_at(T, sq, pj.seg);
            track_obs_preview(T.xy, T.s, k, sq, d, c.x, c.y, sn, cs, px, py);
        }
        // column 7 + 2j (+ 1) is lane j's px (py)
        const int pc = sub - kTrackObsOwn;
        const int src = pc >= 0 && pc < 2 * np ? pc >> 1 : 0;
        const double gx = __shfl(px, src, 64), gy = __shfl(py, src, 64);  // every lane of the half
        const int32_t i = pj.seg < T.n - 2 ? pj.seg : T.n - 2;
        double own[kTrackObsOwn];
        track_obs_own(P, c, pj.t, T.tan[2 * i], T.tan[2 * i + 1], sn, cs, own);
        double gap[kTrackObsGap] = {0.0, 0.0, 0.0};
        if (ok_o) track_obs_gap(P, T.closed, T.L, pj.s, pj.t, c.v, s_o, t_o, v_o, gap);
        const int gc = pc - 2 * np;  // the other car's columns (only with one: else they are pad)
        if (pc < 0) {
#pragma unroll
            for (int j = 0; j < kTrackObsOwn; ++j)
                if (sub == j) val = own[j];
        } else if (pc < 2 * np) {
            val = (pc & 1) ? gy : gx;
        } else if (a.other >= 0 && gc < kTrackObsGap) {
#pragma unroll
            for (int j = 0; j < kTrackObsGap; ++j)
                if (gc == j) val = gap[j];
        }
    }
    if (sub < a.width) a.out[e * a.out_stride + sub] = (float)val;  // one coalesced store per row
}

}  // namespace

hipError_t launch_track_obs(const TrackObsArgs &a, hipStream_t s) {
    if (a.E <= 0) return hipSuccess;
    const int64_t blocks = (a.E + kRaceProjEnvs - 1) / kRaceProjEnvs;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_track_obs, dim3((unsigned)blocks), dim3(64 * kRaceProjEnvs), 0, s, a);
    return hipGetLastError();
}

}  // namespace f110
