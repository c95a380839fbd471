// scan_obs_check.cpp — a stand-alone program over the scan observation's host statement
// (f110_host_scan_obs_push, csrc/f110_host.cpp; the row rule: csrc/f110_scan_obs.h), to be built
// with AddressSanitizer and UBSan on the CPU (scripts/host_check.sh), in the manner of
// host_check.cpp.  Every array has exactly the documented length, so a read or write one element
// past a row, a ring slot or the heads is reported: the ragged-bin shape (B = 1080, K = 7, D = 5)
// and the deepest ring the limits reach (D = 31; D = 32 would need a stride of 31), with strided
// rows, reset flags and both reduces.  Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_scan_obs.h"
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

static void run(int32_t B, int32_t K, int32_t F, int32_t S, int32_t reduce, int32_t keep_mid, int32_t M, int32_t T,
                int64_t E, int64_t row_pad, int64_t out_pad) {
    f110_scan_obs_params P{K, F, S, reduce, keep_mid};
    const int32_t D = scan_obs_depth(P), W = f110_scan_obs_width(&P, B, M, T), in_w = B + M + T;
    CHECK(W == F * K + (keep_mid ? M : 0) + T);
    const int64_t rs = in_w + row_pad, os = W + out_pad;
    // the last row ends where its columns end: no slack behind either array
    std::vector<float> rows((size_t)((E - 1) * rs + in_w)), out((size_t)((E - 1) * os + W), -1.0f);
    std::vector<float> ring((size_t)E * D * K, 0.0f);
    std::vector<int32_t> head((size_t)E, -1);
    std::vector<uint8_t> reset((size_t)E, 0);
    for (int64_t t = 0; t < 2 * D + 3; ++t) {
        for (int64_t e = 0; e < E; ++e)
            for (int32_t c = 0; c < in_w; ++c) rows[(size_t)(e * rs + c)] = value(t, e, c);
        for (int64_t e = 0; e < E; ++e) reset[(size_t)e] = (t == D + 1 && e % 2 == 0) ? 1 : 0;
        CHECK(f110_host_scan_obs_push(&P, E, B, M, T, rows.data(), rs, t < 2 ? nullptr : reset.data(), ring.data(),
                                      head.data(), out.data(), os) == F110_OK);  // (D + 1 >= 2: the flags are seen)
        for (int64_t e = 0; e < E; ++e) {
            const float *o = out.data() + e * os, *r = rows.data() + e * rs;
            CHECK(head[(size_t)e] >= 0 && head[(size_t)e] < D);
            // frame 0 is the slot under the head, and the pooled row itself
            const float *slot = ring.data() + ((size_t)e * D + head[(size_t)e]) * K;
            for (int32_t k = 0; k < K; ++k) {
                CHECK(o[k] == slot[k]);
                CHECK(o[k] == scan_obs_pool(r, scan_obs_edge(k, B, K), scan_obs_edge(k + 1, B, K), reduce));
            }
            if (t == 0 || (t == D + 1 && e % 2 == 0))  // a refill: every frame equal
                for (int32_t j = 1; j < F; ++j)
                    for (int32_t k = 0; k < K; ++k) CHECK(o[j * K + k] == o[k]);
            for (int32_t c = 0; c < W - F * K; ++c) CHECK(o[F * K + c] == r[B + (keep_mid ? 0 : M) + c]);
            for (int64_t c = W; c < os && e + 1 < E; ++c) CHECK(o[c] == -1.0f);  // the pad between strided rows
        }
    }
    CHECK(scan_obs_edge(0, B, K) == 0 && scan_obs_edge(K, B, K) == B);
    for (int32_t k = 0; k < K; ++k) CHECK(scan_obs_edge(k + 1, B, K) > scan_obs_edge(k, B, K));
}

static void check_refusals() {
    f110_scan_obs_params P;
    f110_default_scan_obs_params(&P);
    CHECK(P.n_bins == 108 && P.n_frames == 1 && P.stride == 1 && P.reduce == 0 && P.keep_mid == 1);
    CHECK(f110_scan_obs_width(&P, 1080, 8, 0) == 116 && f110_scan_obs_width(&P, 1080, 8, 20) == 136);
    CHECK(f110_scan_obs_width(&P, 107, 8, 0) == -1 && f110_scan_obs_width(nullptr, 1080, 8, 0) == -1);
    f110_scan_obs_params Q = P;
    Q.n_frames = 3, Q.stride = 15;
    CHECK(scan_obs_depth(Q) == 31 && f110_scan_obs_width(&Q, 1080, 8, 0) == 332);
    Q.stride = 16;  // D = 33
    CHECK(f110_scan_obs_width(&Q, 1080, 8, 0) == -1);
    std::vector<float> rows(1088), out(116), ring(108);
    int32_t head = -1;
    CHECK(f110_host_scan_obs_push(&P, 1, 1080, 8, 0, rows.data(), 1088, nullptr, ring.data(), &head, out.data(), 116) ==
          F110_OK);
    CHECK(f110_host_scan_obs_push(&P, 1, 1080, 8, 0, rows.data(), 1087, nullptr, ring.data(), &head, out.data(), 116) ==
          F110_E_INVALID);
    CHECK(f110_host_scan_obs_push(&P, 1, 1080, 8, 0, rows.data(), 1088, nullptr, ring.data(), &head, out.data(), 115) ==
          F110_E_INVALID);
    CHECK(f110_host_scan_obs_push(&P, 1, 1080, 8, 0, rows.data(), 1088, nullptr, ring.data(), &head, rows.data() + 500,
                                  116) == F110_E_INVALID);  // out inside rows
    head = 1;  // D = 1: no such slot
    CHECK(f110_host_scan_obs_push(&P, 1, 1080, 8, 0, rows.data(), 1088, nullptr, ring.data(), &head, out.data(), 116) ==
          F110_E_INVALID);
}

int main() {
    for (int reduce = 0; reduce <= 1; ++reduce) {
        run(1080, 7, 3, 2, reduce, 1, 8, 20, 3, 0, 0);   // ragged bins, D = 5, packed rows
        run(1080, 7, 3, 2, reduce, 0, 8, 0, 2, 5, 3);    // poses dropped, no tail, strided rows
        run(40, 6, 3, 15, reduce, 1, 4, 0, 3, 1, 0);     // D = 31
        run(33, 33, 7, 5, reduce, 1, 8, 20, 1, 0, 0);    // D = 31 again, identity pooling, one env
        run(5, 3, 1, 1, reduce, 1, 4, 0, 65, 0, 2);      // a tiny row, many envs
    }
    check_refusals();
    std::printf("scan_obs_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
