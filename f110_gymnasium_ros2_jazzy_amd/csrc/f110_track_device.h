// f110_track_device.h — the centerline projection on the device, shared by the kernels that need
// a car's place on the track (private; f110_reward.hip, f110_pursuit.hip, f110_race.hip): the 5 nearest segment
// midpoints of a point (full scan or through the track's grid), CenterlineProgress.project_xy over
// them, and the searchsorted lookup of an arclength.
//
// CenterlineProgress.project_xy asks a cKDTree for the 5 segment midpoints
// nearest to the point and keeps the best orthogonal projection among those
// segments.  Here every lane keeps the 5 nearest of its share of the
// midpoints and a 5-round merge yields the global 5 in ascending
// distance (ties: lower index), the order the candidates are then tried in.
//
// A half-wave (32 lanes) projects one point; every cross-lane step stays inside the half, so the
// two halves of a wave may work on different points, take different paths and leave at different
// times, as long as the lanes of one half stay together.  Everything sits in an anonymous
// namespace: each translation unit gets its own copy, inlined into its kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "f110_task_args.h"

namespace f110 {

namespace {

constexpr int kTop = 5;      // kd.query(p, k=5)

struct Cand {
    double d2;
    int32_t i;
};

__device__ __forceinline__ bool cand_less(double d2a, int32_t ia, double d2b, int32_t ib) {
    return d2a < d2b || (d2a == d2b && ia < ib);
}

__device__ void merge_top(const Cand (&t)[kTop], int sub, Cand out[kTop]);

// Each half-wave (32 lanes) projects its own point: the ego car's on lanes
// 0-31, the opponent's on 32-63, so the two dependent load chains overlap.
// `sub` is the lane within the half; cross-lane steps stay inside it.
constexpr int kHalf = 32;

// The kTop midpoints nearest to (px, py), ascending; every lane of the half gets the same list.
__device__ void nearest_mids(const double *mid, int32_t M, double px, double py, int sub, Cand out[kTop]) {
    Cand t[kTop];
#pragma unroll
    for (int k = 0; k < kTop; ++k) t[k] = Cand{INFINITY, INT32_MAX};
    for (int32_t m = sub; m < M; m += kHalf) {
        const double dx = mid[2 * m] - px, dy = mid[2 * m + 1] - py;
        const double d2 = dx * dx + dy * dy;  // cKDTree's squared euclidean distance
        if (cand_less(d2, m, t[kTop - 1].d2, t[kTop - 1].i)) {
            Cand c{d2, m};
#pragma unroll
            for (int k = 0; k < kTop; ++k)  // insertion into the sorted list
                if (cand_less(c.d2, c.i, t[k].d2, t[k].i)) {
                    const Cand o = t[k];
                    t[k] = c;
                    c = o;
                }
        }
    }
    merge_top(t, sub, out);
}

// The half-wide kTop smallest of the lanes' sorted lists (every lane gets them).
__device__ void merge_top(const Cand (&t)[kTop], int sub, Cand out[kTop]) {
    int head = 0;
#pragma unroll
    for (int r = 0; r < kTop; ++r) {
        double hd = INFINITY;
        int32_t hi = INT32_MAX;
#pragma unroll
        for (int k = 0; k < kTop; ++k)
            if (k == head) {
                hd = t[k].d2;
                hi = t[k].i;
            }
        double bd = hd;
        int32_t bi = hi;
#pragma unroll
        for (int o = kHalf / 2; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int32_t oi = __shfl_xor(bi, o, 64);
            if (cand_less(od, oi, bd, bi)) {
                bd = od;
                bi = oi;
            }
        }
        out[r] = Cand{bd, bi};
        if (hi == bi && bi != INT32_MAX) ++head;  // the winning lane pops its head
    }
}

struct Proj {
    double s, t;
    int32_t seg;  // the segment (or node) s was taken from: seg_at's first guess
};

// np.dot of two 2-vectors / np.linalg.norm of one (OpenBLAS pattern)
__device__ __forceinline__ double bdot(double a0, double a1, double b0, double b1) { return fma(a1, b1, a0 * b0); }

// nearest_mids through the grid: the midpoints of the (2r+1)^2 cells around
// the query, merged as above; the result is final when every midpoint
// outside the block is provably farther than the 5th found one (distance to
// the block's edge, less a margin, above it).  r = 1, then 2, then 4; past
// that the full scan runs.  The same 5 (and order) as the
// full scan.  A grid row's cells are consecutive in cell order, so a block is
// 2r+1 item ranges: their bounds load together, every lane then takes items
// of the concatenated ranges from the cell-ordered midpoint copy.
constexpr int kMaxBlockRows = 9;

__device__ void nearest_mids_grid(const TrackView &T, double px, double py, int sub, Cand out[kTop]) {
    const int32_t M = T.n - 1;
    const double fx = (px - T.gx0) / T.gh, fy = (py - T.gy0) / T.gh;
    bool ok = false;
    // a point off the grid searches from the nearest edge cell: the block's
    // sides on the grid border are clipped (no midpoints beyond them) and
    // the point lies inside every other side, so the bound below still holds
    if (T.cell_start && fx == fx && fy == fy) {
        const int32_t ci = fx < 0.0 ? 0 : (fx >= (double)(T.gnx - 1) ? T.gnx - 1 : (int32_t)fx);
        const int32_t cj = fy < 0.0 ? 0 : (fy >= (double)(T.gny - 1) ? T.gny - 1 : (int32_t)fy);
        for (int32_t r = 1; r <= (kMaxBlockRows - 1) / 2 && !ok; r *= 2) {
            // the block clipped to the grid: a clipped side needs no bound
            const int32_t i0 = ci - r < 0 ? 0 : ci - r, i1 = ci + r >= T.gnx ? T.gnx - 1 : ci + r;
            const int32_t j0 = cj - r < 0 ? 0 : cj - r, j1 = cj + r >= T.gny ? T.gny - 1 : cj + r;
            const int32_t nrow = j1 - j0 + 1;
            int32_t r0[kMaxBlockRows], pre[kMaxBlockRows];
            int32_t K = 0;
#pragma unroll
            for (int t = 0; t < kMaxBlockRows; ++t) {
                r0[t] = 0;
                pre[t] = K;
                if (t < nrow) {
                    const int32_t c = (j0 + t) * T.gnx;
                    r0[t] = T.cell_start[c + i0];
                    K += T.cell_start[c + i1 + 1] - r0[t];
                }
            }
            Cand tp[kTop];
#pragma unroll
            for (int k = 0; k < kTop; ++k) tp[k] = Cand{INFINITY, INT32_MAX};
            for (int32_t j = sub; j < K; j += kHalf) {
                int32_t q = r0[0] + j;
#pragma unroll
                for (int t = 1; t < kMaxBlockRows; ++t)
                    if (t < nrow && j >= pre[t]) q = r0[t] + (j - pre[t]);
                const int32_t m = T.cell_items[q];
                const double dx = T.cell_mid[2 * q] - px, dy = T.cell_mid[2 * q + 1] - py;
                const double d2 = dx * dx + dy * dy;
                if (cand_less(d2, m, tp[kTop - 1].d2, tp[kTop - 1].i)) {
                    Cand cc{d2, m};
#pragma unroll
                    for (int k = 0; k < kTop; ++k)
                        if (cand_less(cc.d2, cc.i, tp[k].d2, tp[k].i)) {
                            const Cand o = tp[k];
                            tp[k] = cc;
                            cc = o;
                        }
                }
            }
            merge_top(tp, sub, out);
            // distance from the query to the block's unclipped edges (a lower
            // bound for every midpoint outside the block), with a margin
            double lb = INFINITY;
            if (ci - r >= 0) lb = fmin(lb, px - (T.gx0 + (double)i0 * T.gh));
            if (ci + r < T.gnx) lb = fmin(lb, T.gx0 + (double)(i1 + 1) * T.gh - px);
            if (cj - r >= 0) lb = fmin(lb, py - (T.gy0 + (double)j0 * T.gh));
            if (cj + r < T.gny) lb = fmin(lb, T.gy0 + (double)(j1 + 1) * T.gh - py);
            const double lbm = lb * (1.0 - 1e-9) - 1e-9;
            ok = out[kTop - 1].i != INT32_MAX && lbm > 0.0 && out[kTop - 1].d2 < lbm * lbm;
        }
    }
    if (!ok) nearest_mids(T.mid, M, px, py, sub, out);  // off the grid or a sparse neighbourhood
}

// CenterlineProgress.project_xy (track_progress.py:58-97)
__device__ Proj project_xy(const TrackView &T, double x, double y, int sub) {
    Cand c[kTop];
    nearest_mids_grid(T, x, y, sub, c);
    bool have = false;
    double bn = 0.0, bs = 0.0, bt = 0.0;
    int32_t bseg = 0;
#pragma unroll
    for (int r = 0; r < kTop; ++r) {
        const int32_t idx = c[r].i;
        if (idx == INT32_MAX) continue;  // fewer than kTop segments
        const double a0 = T.xy[2 * idx], a1 = T.xy[2 * idx + 1];
        const double ab0 = T.xy[2 * idx + 2] - a0, ab1 = T.xy[2 * idx + 3] - a1;
        const double L2 = bdot(ab0, ab1, ab0, ab1);
        if (L2 <= 1e-12) continue;
        const double ap0 = x - a0, ap1 = y - a1;
        double tp = bdot(ap0, ap1, ab0, ab1) / L2;
        tp = tp < 0.0 ? 0.0 : (tp > 1.0 ? 1.0 : tp);  // np.clip (NaN propagates)
        const double pr0 = a0 + tp * ab0, pr1 = a1 + tp * ab1;
        const double s_proj = T.s[idx] + tp * sqrt(L2);
        const double d0 = x - pr0, d1 = y - pr1;
        const double t_signed = bdot(d0, d1, T.nrm[2 * idx], T.nrm[2 * idx + 1]);
        const double nrm = sqrt(bdot(d0, d1, d0, d1));
        if (!have || nrm < bn) {
            have = true;
            bn = nrm;
            bs = s_proj;
            bt = t_signed;
            bseg = idx;
        }
    }
    if (!have) {  // degenerate fallback: nearest node (:93-95)
        double bd = INFINITY;
        int32_t bj = INT32_MAX;
        for (int32_t j = sub; j < T.n; j += kHalf) {
            const double d0 = T.xy[2 * j] - x, d1 = T.xy[2 * j + 1] - y;
            const double d = sqrt(d0 * d0 + d1 * d1);
            if (cand_less(d, j, bd, bj)) {
                bd = d;
                bj = j;
            }
        }
#pragma unroll
        for (int o = kHalf / 2; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int32_t oi = __shfl_xor(bj, o, 64);
            if (cand_less(od, oi, bd, bj)) {
                bd = od;
                bj = oi;
            }
        }
        return Proj{T.s[bj], 0.0, bj};
    }
    return Proj{bs, bt, bseg};
}

// np.searchsorted(s, v, side="right") - 1 clipped to [0, n-2] (rewards.py:112-114, :262-264)
// guess: the segment the projection came from; the answer is checked on it
// and its successor (s is non-decreasing: i is the answer iff s[i] <= v and
// s[i+1] > v or i = n-1) before the binary search runs.
__device__ int32_t seg_at(const TrackView &T, double v, int32_t guess) {
    int32_t lo = 0, hi = T.n;  // first index with s[i] > v
    if (guess >= 0 && guess + 1 < T.n) {
        const double s0 = T.s[guess], s1 = T.s[guess + 1];
        const double s2 = guess + 2 < T.n ? T.s[guess + 2] : INFINITY;
        if (s0 <= v && s1 > v) lo = hi = guess + 1;
        else if (s1 <= v && (guess + 2 >= T.n || s2 > v)) lo = hi = guess + 2;
    }
    while (lo < hi) {
        const int32_t m = (lo + hi) >> 1;
        if (T.s[m] > v) hi = m;
        else lo = m + 1;
    }
    int32_t idx = lo - 1;
    idx = idx < 0 ? 0 : idx;
    return idx > T.n - 2 ? T.n - 2 : idx;
}

}  // namespace
}  // namespace f110
