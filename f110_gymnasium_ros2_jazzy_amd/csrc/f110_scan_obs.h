// f110_scan_obs.h — the row rule of the compact LiDAR observation (private; include/f110.h, "scan
// observation"): sector pooling of a row's range columns, the per-env ring of pooled frames and
// the stacked output row.  k_scan_obs (f110_scan_obs.hip) and f110_host_scan_obs_push
// (f110_host.cpp) both call it.  float32 only: a bin's minimum is a chain of fminf, its mean one sum
// in ascending beam order from the first beam's value and one IEEE division (contraction is off in
// every build of this library), so the device and the host statement agree in every bit.  (fminf's
// choice between -0 and +0 is the platform's; the step's scaled ranges are never negative.)
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_math.h"

namespace f110 {

// Design limits, not measurements.
constexpr int kScanObsMaxFrames = 8;    // n_frames
constexpr int kScanObsMaxStride = 16;   // stride
constexpr int kScanObsMaxDepth = 32;    // the ring depth D = (n_frames - 1) * stride + 1
constexpr int kScanObsMaxBeams = 4096;  // n_beams: a block of k_scan_obs keeps kScanObsEnvs rows of it in LDS
constexpr int kScanObsEnvs = 4;         // envs (= waves) per block of k_scan_obs

static_assert(sizeof(f110_scan_obs_params) == 20, "f110_scan_obs_params: five int32");
static_assert((size_t)kScanObsEnvs * kScanObsMaxBeams * sizeof(float) <= 64 * 1024, "the block's rows fit 64 KiB of LDS");

F110_HD int32_t scan_obs_depth(const f110_scan_obs_params &p) { return (p.n_frames - 1) * p.stride + 1; }

// What every entry refuses of the parameters and the row shape (F110_E_INVALID): null when fine.
inline const char *scan_obs_bad_shape(const f110_scan_obs_params *p, int32_t n_beams, int32_t n_mid, int32_t n_tail) {
    if (!p) return "null params";
    if (n_beams < 1 || n_beams > kScanObsMaxBeams) return "n_beams must be in [1, 4096]";
    if (n_mid < 0 || n_tail < 0 || n_mid > (1 << 20) || n_tail > (1 << 20)) return "n_mid and n_tail must be in [0, 2^20]";
    if (p->n_bins < 1 || p->n_bins > n_beams) return "n_bins must be in [1, n_beams]";
    if (p->n_frames < 1 || p->n_frames > kScanObsMaxFrames) return "n_frames must be in [1, 8]";
    if (p->stride < 1 || p->stride > kScanObsMaxStride) return "stride must be in [1, 16]";
    if (scan_obs_depth(*p) > kScanObsMaxDepth) return "the ring depth (n_frames - 1) * stride + 1 must not exceed 32";
    if (p->reduce != 0 && p->reduce != 1) return "reduce must be 0 (min) or 1 (mean)";
    if (p->keep_mid != 0 && p->keep_mid != 1) return "keep_mid must be 0 or 1";
    return nullptr;
}

// [F*K | M if keep_mid | T]
inline int32_t scan_obs_width(const f110_scan_obs_params &p, int32_t n_mid, int32_t n_tail) {
    return p.n_frames * p.n_bins + (p.keep_mid ? n_mid : 0) + n_tail;
}

// What a push refuses of its arrays: null when fine.  in_width = B + M + T, width = scan_obs_width.
inline const char *scan_obs_bad_push(int64_t n_envs, int32_t in_width, int32_t width, const float *rows,
                                     int64_t row_stride, const float *out, int64_t out_stride) {
    if (!rows || !out) return "null rows or out";
    if (row_stride < in_width) return "row_stride below n_beams + n_mid + n_tail";
    if (out_stride < width) return "out_stride below the width";
    const float *rows_end = rows + (n_envs - 1) * row_stride + in_width;
    const float *out_end = out + (n_envs - 1) * out_stride + width;
    if (out < rows_end && rows < out_end) return "out overlaps rows";
    return nullptr;
}

// Bin j covers beams [scan_obs_edge(j), scan_obs_edge(j + 1)): never empty while K <= B.
F110_HD int32_t scan_obs_edge(int32_t j, int32_t B, int32_t K) { return (int32_t)(((int64_t)j * B) / K); }

// One bin's pooled value over beams [lo, hi) of v.
F110_HD float scan_obs_pool(const float *v, int32_t lo, int32_t hi, int32_t reduce) {
    float acc = v[lo];
    if (reduce == 0) {
        for (int32_t b = lo + 1; b < hi; ++b) acc = fminf(acc, v[b]);
        return acc;
    }
    for (int32_t b = lo + 1; b < hi; ++b) acc = acc + v[b];
    return acc / (float)(hi - lo);
}

// The ring's step: an empty ring (head -1) or a reset row refills (every slot takes the frame, head
// 0); otherwise the head moves on by one slot, which alone takes the frame.
F110_HD int32_t scan_obs_advance(int32_t head, int reset, int32_t D, bool &refill) {
    refill = head < 0 || reset != 0;
    return refill ? 0 : (head + 1) % D;
}

// The slot of frame j (0 = newest) under head `head`: (head - j*S) mod D.
F110_HD int32_t scan_obs_slot(int32_t head, int32_t j, int32_t S, int32_t D) {
    return ((head - j * S) % D + D) % D;
}

}  // namespace f110
