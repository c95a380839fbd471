// f110_sensor.h — the row rule of the sensor randomization (private; include/f110.h, "sensor
// randomization"): the per-env parameter draw, the counter rule and what one range, pose or other
// column of a full observation row becomes.  k_sensor (f110_sensor.hip) and f110_host_sensor_apply
// (f110_host.cpp) both call it.  float32 and integers only, in a fixed order, no libm call but
// rintf, no hardware transcendental (contraction is off in every build of this library), so the
// device and the host statement agree in every bit.
//
// Draws: Philox4x32-10 (f110_rng.h) under param_draw's key of (seed, global env id):
//   k0 = (u32)seed ^ (u32)env,  k1 = (u32)(seed >> 32) ^ (u32)(env >> 32) ^ 0xA5A5A5A5
//   parameter block j = 0..2 of an episode   counter (j, 0, 0x5E250, episode)
//   column block of an apply                 counter (column, step, 0x5E251, episode)
// (the tag sits in counter word 2, where param_draw keeps 0xD0A17, spawn_draw 0x5BA3E and
// spawn_draws 0x5FA17: no two streams of one key meet).  column is the row's own column index: a
// beam b < B, or B + m for middle column m.  episode and step are the env's counters below.
//   parameter block 0: scale, noise_abs, noise_rel, dropout      (words x, y, z, w)
//   parameter block 1: blackout width, blackout start, quant, pose_xy
//   parameter block 2: pose_theta (word x)
//   a real parameter   lo + u * (hi - lo),  u = (float)(word >> 8) * 2^-24   (hi == lo gives lo)
//   an integer in [0, n)   (word * n) >> 32   (32 x 32 -> 64 multiply-high)
//   column block: z = (float)(S - 1530) * (1/256), S the sum of the 12 bytes of words x, y, z
//   (mean 0, std sqrt(65535)/256, |z| <= 1530/256); the dropout bits are word w >> 8.
#pragma once

#include <math.h>
#include <stdint.h>

#include <cmath>

#include "../../include/f110.h"
#include "f110_math.h"
#include "f110_rng.h"

namespace f110 {

// Design limits, not measurements.
constexpr int kSensorMaxBeams = 4096;  // n_beams (the blackout width and start stay exact in float32)
constexpr int kSensorThreads = 256;    // threads of k_sensor's block, one block per env
constexpr uint32_t kSensorParamTag = 0x5E250u, kSensorDrawTag = 0x5E251u;
constexpr float kSensorPi = 3.14159274101257324f;     // (float)pi
constexpr float kSensorTwoPi = 6.28318548202514648f;  // (float)(2 pi)

static_assert(sizeof(f110_sensor_params) == 64, "f110_sensor_params: eight (lo, hi) float pairs");

// One env's drawn parameters, in the row's own units (f110_sensor_arrays' parameter row: 10 floats).
struct SensorRow {
    float scale;       // range factor
    float noise_abs;   // additive sigma / range_max
    float noise_rel;   // proportional sigma
    float dropout;     // per-beam, per-step probability of no return
    float black_w;     // blocked sector: width in beams ...
    float black_s;     // ... and first beam (both whole numbers)
    float quant;       // quantization step / range_max, 0 = off
    float pose_xy;     // sigma of the x and y columns, metres
    float pose_theta;  // sigma of the theta columns, radians
    float drop_thr;    // floor(dropout * 2^24): a beam drops when its 24 bits are below it
};
constexpr int kSensorRowFloats = 10;
static_assert(sizeof(SensorRow) == kSensorRowFloats * sizeof(float), "SensorRow: ten floats");

struct SensorKey { uint32_t k0, k1; };

F110_HD SensorKey sensor_key(uint64_t seed, uint64_t env) {
    return {(uint32_t)seed ^ (uint32_t)env, (uint32_t)(seed >> 32) ^ (uint32_t)(env >> 32) ^ 0xA5A5A5A5u};
}

F110_HD float sensor_uniform(const float r[2], uint32_t word) {
    const float u = (float)(word >> 8) * (1.0f / 16777216.0f);  // [0, 1), 24 bits: exact
    return r[0] + u * (r[1] - r[0]);
}

F110_HD uint32_t sensor_below(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * n) >> 32); }  // [0, n)

// The parameters of (key, episode).  Metre-valued range parameters (noise_abs, quant) become the
// row's normalized units here, once per episode: one IEEE division by range_max each.
F110_HD SensorRow sensor_draw_row(SensorKey k, uint32_t episode, const f110_sensor_params &p, int32_t B,
                                  float range_max) {
    const U4 a = philox(U4{0u, 0u, kSensorParamTag, episode}, k.k0, k.k1);
    const U4 b = philox(U4{1u, 0u, kSensorParamTag, episode}, k.k0, k.k1);
    const U4 c = philox(U4{2u, 0u, kSensorParamTag, episode}, k.k0, k.k1);
    SensorRow r;
    r.scale = sensor_uniform(p.scale, a.x);
    r.noise_abs = sensor_uniform(p.noise_abs, a.y) / range_max;
    r.noise_rel = sensor_uniform(p.noise_rel, a.z);
    r.dropout = sensor_uniform(p.dropout, a.w);
    r.drop_thr = (float)(uint32_t)(r.dropout * 16777216.0f);  // <= 2^24: exact in float32
    const uint32_t w_lo = (uint32_t)p.blackout[0], w_hi = (uint32_t)p.blackout[1];
    const uint32_t w = w_lo + sensor_below(b.x, w_hi - w_lo + 1u);
    r.black_w = (float)w;
    r.black_s = (float)sensor_below(b.y, (uint32_t)B - w + 1u);  // every start that keeps it inside the scan
    r.quant = sensor_uniform(p.quant, b.z) / range_max;
    r.pose_xy = sensor_uniform(p.pose_xy, b.w);
    r.pose_theta = sensor_uniform(p.pose_theta, c.x);
    return r;
}

// The counter rule of one apply: an env that has had none yet (episode < 0) or whose reset flag is
// set starts an episode (the next episode number, step 0: its parameters are redrawn); any other
// apply is the episode's next step.  Both counters wrap (2^31 episodes, 2^32 steps).
F110_HD bool sensor_advance(int32_t &episode, int32_t &step, int reset) {
    const bool start = episode < 0 || reset != 0;
    if (start) {
        episode = (int32_t)(((uint32_t)episode + 1u) & 0x7fffffffu);
        step = 0;
    } else {
        step = (int32_t)((uint32_t)step + 1u);
    }
    return start;
}

// Which draws a row needs at all (env-uniform): with neither, no block is computed.
F110_HD bool sensor_beam_draws(const SensorRow &r) {
    return r.noise_abs > 0.0f || r.noise_rel > 0.0f || r.drop_thr > 0.0f;
}

F110_HD U4 sensor_block(SensorKey k, uint32_t episode, uint32_t step, uint32_t column) {
    return philox(U4{column, step, kSensorDrawTag, episode}, k.k0, k.k1);
}

F110_HD float sensor_normal(const U4 &r) {
    const uint32_t m = 0x00ff00ffu;  // two byte sums per word pair, 6 * 255 each at the most
    const uint32_t t = (r.x & m) + ((r.x >> 8) & m) + (r.y & m) + ((r.y >> 8) & m) + (r.z & m) + ((r.z >> 8) & m);
    const int32_t S = (int32_t)((t & 0xffffu) + (t >> 16));
    return (float)(S - 1530) * (1.0f / 256.0f);
}

// Beam b of value d (the row's normalized range).  k: sensor_block of the beam's column, read only
// where sensor_beam_draws(r).  A step whose parameter is the identity's is skipped, not computed
// with a zero, so the identity parameters return d's own bits (a negative zero, a subnormal).
F110_HD float sensor_beam(float d, int32_t b, const SensorRow &r, const U4 &k) {
    d = d * r.scale;
    if (r.noise_abs > 0.0f || r.noise_rel > 0.0f) d = d + sensor_normal(k) * (r.noise_abs + r.noise_rel * d);
    if (r.quant > 0.0f) d = r.quant * rintf(d / r.quant);
    if (r.drop_thr > 0.0f && (k.w >> 8) < (uint32_t)r.drop_thr) d = 1.0f;  // no return: max range
    const int32_t s = (int32_t)r.black_s;
    if (b >= s && b < s + (int32_t)r.black_w) d = 0.0f;  // blocked
    return d < 0.0f ? 0.0f : (d > 1.0f ? 1.0f : d);
}

// Middle column m (group m / 4: x, y, theta, collision) of value v; k: sensor_block of column B + m,
// read only where the column's sigma is positive.
F110_HD bool sensor_pose_draws(const SensorRow &r, int32_t m) {
    return (m & 3) < 2 ? r.pose_xy > 0.0f : ((m & 3) == 2 && r.pose_theta > 0.0f);
}

F110_HD float sensor_pose(float v, int32_t m, const SensorRow &r, const U4 &k) {
    if (!sensor_pose_draws(r, m)) return v;
    if ((m & 3) < 2) return v + sensor_normal(k) * r.pose_xy;
    float t = v + sensor_normal(k) * r.pose_theta;
    if (t > kSensorPi) t = t - kSensorTwoPi;  // one turn back into [-pi, pi]
    else if (t < -kSensorPi) t = t + kSensorTwoPi;
    return t;
}

// ---- what the entries refuse (F110_E_INVALID): null when fine ---------------------------------
inline const char *sensor_bad_params(const f110_sensor_params *p, int32_t n_beams) {
    if (!p) return "null params";
    const float *pairs[8] = {p->scale, p->noise_abs, p->noise_rel, p->dropout, p->blackout, p->quant, p->pose_xy, p->pose_theta};
    for (const float *r : pairs) {
        if (!std::isfinite(r[0]) || !std::isfinite(r[1])) return "a bound that is not finite";
        if (r[0] > r[1]) return "a range with lo > hi";
    }
    if (!(p->scale[0] > 0.0f)) return "scale must be > 0";
    if (p->noise_abs[0] < 0.0f || p->noise_rel[0] < 0.0f || p->pose_xy[0] < 0.0f || p->pose_theta[0] < 0.0f)
        return "a sigma (noise_abs, noise_rel, pose_xy, pose_theta) must be >= 0";
    if (p->quant[0] < 0.0f) return "quant must be >= 0";
    if (p->dropout[0] < 0.0f || p->dropout[1] > 1.0f) return "dropout must be in [0, 1]";
    if (p->blackout[0] < 0.0f || p->blackout[1] > (float)n_beams) return "blackout must be in [0, n_beams]";
    if (p->blackout[0] != rintf(p->blackout[0]) || p->blackout[1] != rintf(p->blackout[1]))
        return "blackout must be whole beams";
    return nullptr;
}

inline const char *sensor_bad_shape(const f110_sensor_params *p, int64_t n_envs, int32_t n_beams, int32_t n_mid,
                                    int32_t n_tail, float range_max, int64_t env_offset) {
    if (n_envs < 1 || n_envs >= (int64_t)1 << 31) return "n_envs must be positive (and below 2^31)";
    if (n_beams < 1 || n_beams > kSensorMaxBeams) return "n_beams must be in [1, 4096]";
    if (n_mid < 0 || n_mid > (1 << 20) || n_mid % 4 != 0) return "n_mid must be a multiple of 4 in [0, 2^20]";
    if (n_tail < 0 || n_tail > (1 << 20)) return "n_tail must be in [0, 2^20]";
    if (!(range_max > 0.0f) || !std::isfinite(range_max)) return "range_max must be > 0 and finite";
    if (env_offset < 0) return "env_offset must be >= 0";
    return sensor_bad_params(p, n_beams);
}

// What an apply refuses of its arrays.  out is rows itself (same pointer, same stride: every column
// is read and written by one lane) or shares no float with it.
inline const char *sensor_bad_apply(int64_t n_envs, int32_t width, const float *rows, int64_t row_stride,
                                    const float *out, int64_t out_stride) {
    if (!rows || !out) return "null rows or out";
    if (row_stride < width) return "row_stride below n_beams + n_mid + n_tail";
    if (out_stride < width) return "out_stride below the width";
    if (out == rows && out_stride == row_stride) return nullptr;
    const float *rows_end = rows + (n_envs - 1) * row_stride + width;
    const float *out_end = out + (n_envs - 1) * out_stride + width;
    if (out < rows_end && rows < out_end) return "out overlaps rows in part (it must be rows itself or disjoint)";
    return nullptr;
}

}  // namespace f110
