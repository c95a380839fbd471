// repeat_check.cpp — a stand-alone program over the action-repeat host hooks of libf110.so
// (f110_host_repeat_hold / f110_host_repeat_push, csrc/f110_host.cpp), to be built with
// AddressSanitizer and UBSan on the CPU (scripts/host_check.sh).  It drives the two functions over a
// few hundred seeded steps with buffers of exactly the documented length, so an index that strays is
// reported by the sanitizer, and checks the cheap invariants of what they return against a rule kept
// here in its plainest form.  Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        ++g_checks;                                                           \
        if (!(cond)) {                                                        \
            ++g_failed;                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
        }                                                                     \
    } while (0)

static uint64_t g_state = 0;
static uint32_t rnd() {  // splitmix64's high word
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static double unit() { return rnd() / 4294967296.0; }

static void run(int N, int D, int A, int K, double gamma, int T, uint64_t seed) {
    g_state = seed;
    const size_t n = (size_t)N;
    std::vector<int32_t> k(n, 0), want_k(n, 0);
    std::vector<double> ret(n, 0.0), want_ret(n, 0.0), reward(n);
    std::vector<float> s_obs(n * D, 0.0f), s_act(n * A, 0.0f), obs(n * D), act(n * A), next_obs(n * D), held(n * A, 0.0f);
    std::vector<uint8_t> decision(n), term(n), trunc(n), reset(n, 0), prev_end(n, 0);
    std::vector<float> o_obs(n * D), o_act(n * A), o_rew(n), o_next(n * D), o_done(n);
    std::vector<double> pw((size_t)K + 1, 1.0);
    for (int i = 1; i <= K; ++i) pw[(size_t)i] = pw[(size_t)i - 1] * gamma;
    const double pe = K >= 16 ? 0.004 : 0.05;  // long blocks need long episodes to run to K
    int64_t emitted = 0, pushed = 0, full = 0;
    for (int t = 0; t < T; ++t) {
        for (auto &x : obs) x = (float)(unit() - 0.5);
        for (auto &x : act) x = (float)(unit() - 0.5);
        for (auto &x : next_obs) x = (float)(unit() - 0.5);
        for (size_t e = 0; e < n; ++e) {
            reward[e] = unit() < 0.02 ? -0.0 : unit() * 4.0 - 2.0;
            reset[e] = prev_end[e] || unit() < 0.01;
            const double u = unit();
            term[e] = !reset[e] && u < pe;
            trunc[e] = !reset[e] && u > 0.6 * pe && u < 1.6 * pe;
            prev_end[e] = term[e] || trunc[e];
        }
        const std::vector<float> policy = act;
        CHECK(f110_host_repeat_hold(N, D, A, k.data(), s_obs.data(), s_act.data(), obs.data(), act.data(),
                                    t % 2 ? decision.data() : nullptr) == F110_OK);
        for (size_t e = 0; e < n; ++e) {
            if (t % 2) CHECK(decision[e] == (want_k[e] == 0 ? 1 : 0));
            for (int j = 0; j < A; ++j) {
                if (want_k[e] == 0) held[e * A + j] = policy[e * A + j];
                CHECK(act[e * A + j] == held[e * A + j]);
                CHECK(s_act[e * A + j] == held[e * A + j]);
            }
            if (K == 1) CHECK(want_k[e] == 0);
        }
        int64_t count = -1;
        CHECK(f110_host_repeat_push(N, K, gamma, D, A, t % 3 ? N : 0, k.data(), ret.data(), s_obs.data(), s_act.data(),
                                    reward.data(), next_obs.data(), term.data(), t % 5 ? trunc.data() : nullptr,
                                    reset.data(), o_obs.data(), o_act.data(), o_rew.data(), o_next.data(), o_done.data(),
                                    &count) == F110_OK);
        int64_t row = 0;
        for (size_t e = 0; e < n; ++e) {
            const bool tr = t % 5 ? trunc[e] != 0 : false;
            if (reset[e]) {
                want_k[e] = 0;
                CHECK(k[e] == 0);
                continue;
            }
            ++pushed;
            want_ret[e] = want_k[e] == 0 ? reward[e] : want_ret[e] + pw[(size_t)want_k[e]] * reward[e];
            want_k[e] += 1;
            if (term[e] || tr || want_k[e] == K) {
                CHECK(row < count);
                if (row < count) {
                    CHECK(o_rew[(size_t)row] == (float)want_ret[e] &&
                          std::signbit(o_rew[(size_t)row]) == std::signbit((float)want_ret[e]));
                    CHECK(o_done[(size_t)row] == (term[e] ? 1.0f : (float)(1.0 - pw[(size_t)want_k[e] - 1])));
                    for (int j = 0; j < D; ++j) {
                        CHECK(o_obs[(size_t)row * D + j] == s_obs[e * D + j]);
                        CHECK(o_next[(size_t)row * D + j] == next_obs[e * D + j]);
                    }
                    for (int j = 0; j < A; ++j) CHECK(o_act[(size_t)row * A + j] == held[e * A + j]);
                }
                ++row;
                full += !term[e] && !tr;
                want_k[e] = 0;
            }
            CHECK(k[e] == want_k[e] && k[e] < K);
            if (k[e] > 0) CHECK(ret[e] == want_ret[e]);
        }
        CHECK(row == count);
        emitted += count;
    }
    CHECK(emitted > 0 && emitted <= pushed && full > 0);
    if (K == 1) CHECK(emitted == pushed);
}

static void check_validation() {
    int32_t k[2] = {0, 0};
    double ret[2] = {0, 0}, reward[2] = {0, 0};
    float row[8] = {0}, out[8] = {0}, o1[2], o2[2];
    uint8_t z[2] = {0, 0};
    int64_t count = 0;
    auto push = [&](int64_t n, int32_t K, double gamma, int64_t cap) {
        return f110_host_repeat_push(n, K, gamma, 4, 2, cap, k, ret, row, row, reward, row, z, nullptr, z, out, out, o1, out,
                                     o2, &count);
    };
    CHECK(push(2, 3, 0.99, 2) == F110_OK);
    CHECK(push(2, 0, 0.99, 0) == F110_E_INVALID);
    CHECK(push(2, 65, 0.99, 0) == F110_E_INVALID);
    CHECK(push(2, 3, 1.5, 0) == F110_E_INVALID);
    CHECK(push(2, 3, -0.1, 0) == F110_E_INVALID);
    CHECK(push(2, 3, std::numeric_limits<double>::quiet_NaN(), 0) == F110_E_INVALID);
    CHECK(push(2, 3, 0.99, 1) == F110_E_INVALID);
    CHECK(push(0, 3, 0.99, 0) == F110_E_INVALID);
    CHECK(f110_host_repeat_hold(0, 4, 2, k, row, row, row, row, nullptr) == F110_E_INVALID);
    CHECK(f110_host_repeat_hold(2, 4, 2, nullptr, row, row, row, row, nullptr) == F110_E_INVALID);
}

int main() {
    const double gammas[4] = {0.99, 0.5, 1.0, 0.0};
    int g = 0;
    for (int K : {1, 2, 3, 7, 64})
        for (const auto &nd : {std::pair<int, int>{1, 1}, {5, 6}, {33, 8}})
            run(nd.first, nd.second, 2, K, gammas[g++ % 4], K == 64 ? 400 : 200, 1000u * (unsigned)K + (unsigned)nd.first);
    run(3, 5, 1, 64, 1.0, 300, 7);
    check_validation();
    std::printf("repeat_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
