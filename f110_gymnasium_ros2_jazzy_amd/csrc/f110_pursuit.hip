// f110_pursuit.hip — the pure-pursuit centerline opponent on the device (include/f110.h,
// "pure-pursuit opponent"): every car aims at the centerline point one lookahead ahead of its own
// projection.  No reference counterpart (train_ddpg.py races gap_follow_action only); the
// projection is the reward's (f110_track_device.h), the row rule f110_pursuit.h's, which
// f110_host_pure_pursuit states on the host.
//
// As in k_reward a half-wave (32 lanes) owns one car: the nearest-midpoint search spreads over its
// lanes and every cross-lane step stays inside it.  A wave takes two rows, so their two dependent
// load chains (grid bounds -> midpoints -> segment ends) overlap.  Nothing below leaves a half
// divided: a row is skipped (its mask is 0, or its pose is not finite) by all 32 lanes or by none,
// and the upper half of an odd last wave rides along on the last row and stores nothing, so every
// shuffle a half executes has all of that half's lanes in it.  The arithmetic after the projection
// is scalar per car: lane 0 of the half computes it and writes the row with plain vector stores
// (one writer per element).  One-wave blocks, no LDS, no barrier, no atomics, no allocation.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_pursuit.h"
#include "f110_task_args.h"
#include "f110_track_device.h"

namespace f110 {

namespace {

constexpr int kPpRows = 64 / kHalf;  // rows per wave (= per block)

}  // namespace

__global__ void __launch_bounds__(64) k_pursuit(PursuitArgs a) {
    const int lane = threadIdx.x & 63;
    const int sub = lane & (kHalf - 1);
    const int64_t row = (int64_t)blockIdx.x * kPpRows + (lane >> 5);
    const bool tail = row >= a.M;  // (the grid has no block whose first row is past the end)
    const int64_t m = tail ? a.M - 1 : row;
    const bool writer = sub == 0 && !tail;
    if (a.row_mask && a.row_mask[m] == 0) return;  // the whole half: no shuffle of it is left behind
    const float *p = a.poses + m * a.pose_stride;
    const double x = (double)p[0], y = (double)p[1], yaw = (double)p[2];
    float *act = a.actions + m * a.action_stride;
    double *aux = a.aux ? a.aux + 4 * m : nullptr;
    if (!(isfinite(x) && isfinite(y) && isfinite(yaw))) {  // half-uniform; the projection needs a finite point
        if (writer) {
            act[0] = 0.0f;
            act[1] = 0.0f;
            if (aux) aux[0] = aux[1] = aux[2] = aux[3] = (double)NAN;
        }
        return;
    }
    const TrackView &T = a.track;
    const Proj pj = project_xy(T, x, y, sub);  // every lane of the half gets the same result
    if (!writer) return;
    const double sq = pursuit_query(a.p, pj.s, T.closed, T.L);
    const int32_t i = seg_at(T, sq, pj.seg);
    const PursuitAction r = pursuit_action(a.p, T.xy, T.s, i, sq, x, y, yaw, a.row_speed ? a.row_speed[m] : a.p.speed);
    act[0] = (float)r.steer;
    act[1] = (float)r.v;
    if (aux) {
        aux[0] = pj.s;
        aux[1] = pj.t + 0.0;  // a zero offset as +0, np.dot's zero (bdot's fma keeps the sign of -0 + -0)
        aux[2] = r.tx;
        aux[3] = r.ty;
    }
}

hipError_t launch_pursuit(const PursuitArgs &a, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    const int64_t blocks = (a.M + kPpRows - 1) / kPpRows;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pursuit, dim3((unsigned)blocks), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace f110
