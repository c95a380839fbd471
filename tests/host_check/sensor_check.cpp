// sensor_check.cpp — a stand-alone program over the sensor randomization's host statement
// (f110_host_sensor_apply, csrc/f110_host.cpp; the row rule: csrc/f110_sensor.h), to be built with
// AddressSanitizer and UBSan on the CPU (scripts/host_check.sh), in the manner of
// scan_obs_check.cpp.  Every array has exactly the documented length, so a read or write one element
// past a row, a parameter row, a counter or the mask is reported: shapes around one wave's 64
// columns, strided rows, in place and disjoint, every parameter active, reset flags, a mask, the
// widest blackout, and counters at their wrap.  Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_sensor.h"
#include "../../include/f110.h"
#include "../../include/f110_debug.h"

using namespace f110;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        ++g_checks;                                                           \
        if (!(cond)) {                                                        \
            ++g_failed;                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
        }                                                                     \
    } while (0)

static float value(int64_t t, int64_t e, int32_t c) { return (float)((t * 131 + e * 17 + c * 7) % 97) / 97.0f; }

static f110_sensor_params active(int32_t B) {
    f110_sensor_params P;
    f110_default_sensor_params(&P);
    P.scale[0] = 0.9f, P.scale[1] = 1.1f;
    P.noise_abs[0] = 0.01f, P.noise_abs[1] = 0.3f;
    P.noise_rel[0] = 0.0f, P.noise_rel[1] = 0.05f;
    P.dropout[0] = 0.0f, P.dropout[1] = 0.3f;
    P.blackout[0] = 0.0f, P.blackout[1] = (float)B;  // up to the whole scan
    P.quant[0] = 0.0f, P.quant[1] = 0.1f;
    P.pose_xy[0] = 0.0f, P.pose_xy[1] = 0.1f;
    P.pose_theta[0] = 0.0f, P.pose_theta[1] = 0.5f;
    return P;
}

static void run(int32_t B, int32_t M, int32_t T, int64_t E, int64_t row_pad, bool in_place, bool masked) {
    const f110_sensor_params P = active(B);
    const int32_t W = B + M + T;
    const int64_t rs = W + row_pad, os = in_place ? rs : W + 2;
    // the last row ends where its columns end: no slack behind either array
    std::vector<float> rows((size_t)((E - 1) * rs + W)), other((size_t)((E - 1) * os + W), -1.0f);
    std::vector<float> par((size_t)E * kSensorRowFloats, 0.0f);
    std::vector<int32_t> episode((size_t)E, -1), step((size_t)E, 0);
    std::vector<uint8_t> reset((size_t)E, 0), mask((size_t)E, 1);
    for (int64_t e = 0; e < E; ++e) mask[(size_t)e] = e % 3 != 1;
    float *out = in_place ? rows.data() : other.data();
    for (int64_t t = 0; t < 5; ++t) {
        for (int64_t e = 0; e < E; ++e)
            for (int32_t c = 0; c < W; ++c) rows[(size_t)(e * rs + c)] = value(t, e, c);
        for (int64_t e = 0; e < E; ++e) reset[(size_t)e] = (t == 3 && e % 2 == 0) ? 1 : 0;
        CHECK(f110_host_sensor_apply(&P, E, B, M, T, 30.0f, 0x123456789abcdefull, 1000, masked ? mask.data() : nullptr,
                                     rows.data(), rs, t < 1 ? nullptr : reset.data(), par.data(), episode.data(),
                                     step.data(), out, os) == F110_OK);
        for (int64_t e = 0; e < E; ++e) {
            const float *o = out + e * os;
            const SensorRow &r = reinterpret_cast<const SensorRow *>(par.data())[e];
            const bool again = t >= 3 && e % 2 == 0;
            CHECK(episode[(size_t)e] == (again ? 1 : 0) && step[(size_t)e] == (again ? t - 3 : t));
            CHECK(r.black_w >= 0.0f && r.black_s >= 0.0f && r.black_s + r.black_w <= (float)B);
            CHECK(r.scale >= 0.9f && r.scale <= 1.1f && r.drop_thr <= 16777216.0f);
            for (int32_t b = 0; b < B; ++b) CHECK(o[b] >= 0.0f && o[b] <= 1.0f);
            for (int32_t m = 2; m < M; m += 4) CHECK(std::fabs(o[B + m]) <= kSensorPi);
            if (masked && !mask[(size_t)e])
                for (int32_t c = 0; c < W; ++c) CHECK(o[c] == value(t, e, c));
            for (int32_t m = 3; m < M; m += 4) CHECK(o[B + m] == value(t, e, B + m));         // collision
            for (int32_t c = B + M; c < W; ++c) CHECK(o[c] == value(t, e, c));                 // the tail
            if (!in_place)
                for (int64_t c = W; c < os && e + 1 < E; ++c) CHECK(o[c] == -1.0f);            // the pad between rows
        }
    }
}

static void check_wrap_and_refusals() {
    f110_sensor_params P = active(8);
    std::vector<float> rows(8 + 4, 0.5f), out(8 + 4), par(kSensorRowFloats);
    int32_t episode = 0x7fffffff, step = -1;  // the last episode number, step 2^32 - 1
    uint8_t flag = 0;
    CHECK(f110_host_sensor_apply(&P, 1, 8, 4, 0, 30.0f, 1, 0, nullptr, rows.data(), 12, &flag, par.data(), &episode, &step,
                                 out.data(), 12) == F110_OK);
    CHECK(episode == 0x7fffffff && step == 0);
    flag = 1;
    CHECK(f110_host_sensor_apply(&P, 1, 8, 4, 0, 30.0f, 1, 0, nullptr, rows.data(), 12, &flag, par.data(), &episode, &step,
                                 out.data(), 12) == F110_OK);
    CHECK(episode == 0 && step == 0);
    f110_sensor_params I;
    f110_default_sensor_params(&I);
    rows[0] = 0.0f, rows[1] = 1.0f, rows[2] = 1e-42f;
    CHECK(f110_host_sensor_apply(&I, 1, 8, 4, 0, 30.0f, 1, 0, nullptr, rows.data(), 12, &flag, par.data(), &episode, &step,
                                 out.data(), 12) == F110_OK);  // (the flag: the identity's row is drawn)
    for (int c = 0; c < 12; ++c) CHECK(out[(size_t)c] == rows[(size_t)c]);
    CHECK(f110_host_sensor_apply(&I, 1, 8, 4, 0, 30.0f, 1, 0, nullptr, rows.data(), 11, nullptr, par.data(), &episode, &step,
                                 out.data(), 12) == F110_E_INVALID);
    CHECK(f110_host_sensor_apply(&I, 1, 8, 4, 0, 30.0f, 1, 0, nullptr, rows.data(), 12, nullptr, par.data(), &episode, &step,
                                 rows.data() + 1, 12) == F110_E_INVALID);  // a partial overlap
    CHECK(f110_host_sensor_apply(&I, 1, 8, 3, 0, 30.0f, 1, 0, nullptr, rows.data(), 12, nullptr, par.data(), &episode, &step,
                                 out.data(), 12) == F110_E_INVALID);
    I.blackout[1] = 9.0f;
    CHECK(f110_host_check_sensor_params(&I, 8) == F110_E_INVALID && f110_host_check_sensor_params(&I, 9) == F110_OK);
}

int main() {
    for (int in_place = 0; in_place <= 1; ++in_place)
        for (int masked = 0; masked <= 1; ++masked) {
            run(1080, 8, 20, 3, 0, in_place, masked);  // the env's row, packed
            run(1080, 8, 0, 2, 5, in_place, masked);   // no tail, strided rows
            run(65, 4, 5, 4, 1, in_place, masked);     // one column past a wave
            run(63, 8, 0, 3, 0, in_place, masked);
            run(1, 4, 0, 5, 2, in_place, masked);      // one beam
            run(4096, 0, 0, 1, 0, in_place, masked);   // the widest scan, no poses
        }
    check_wrap_and_refusals();
    std::printf("sensor_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
