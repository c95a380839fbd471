// host_check.cpp — a stand-alone program over the pure host code of libf110.so (csrc/f110_host.cpp),
// to be built with AddressSanitizer and UBSan on the CPU (scripts/host_check.sh).  It calls the host
// functions at small and awkward sizes with buffers of exactly the documented length, so an index
// that strays is reported by the sanitizer, and checks the cheap invariants of what they return.
// Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_host.h"
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

// ---- EDT and the two table builders --------------------------------------------
static void check_maps() {
    const int shapes[4][2] = {{1, 1}, {1, 7}, {5, 3}, {33, 17}};
    for (const auto &hw : shapes) {
        const int H = hw[0], W = hw[1];
        std::vector<uint8_t> free_mask((size_t)H * W);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) free_mask[(size_t)r * W + c] = (r * 7 + c * 3) % 5 == 0 ? 0 : 1;
        std::vector<uint32_t> k((size_t)H * W);
        CHECK(f110_edt_k(free_mask.data(), H, W, k.data()) == F110_OK);
        for (int r = 0; r < H; ++r)  // against the definition
            for (int c = 0; c < W; ++c) {
                int64_t best = std::numeric_limits<int64_t>::max();
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        if (!free_mask[(size_t)y * W + x]) {
                            const int64_t d = (int64_t)(y - r) * (y - r) + (int64_t)(x - c) * (x - c);
                            best = d < best ? d : best;
                        }
                CHECK((int64_t)k[(size_t)r * W + c] == best);
            }
        const double res = 0.25;
        for (int kind = 0; kind < 2; ++kind)
            for (int pad : {0, 9}) {
                int64_t meta[3] = {0, 0, 0};
                const int64_t n = f110_host_map_table(k.data(), H, W, res, kind, pad, nullptr, 0, meta);
                if (kind == 1 && pad == 0) {
                    CHECK(n == 0 && meta[2] == -1);
                    continue;
                }
                CHECK(n > 0 && meta[2] == meta[0] * meta[1] * 8 && n == meta[0] * meta[1] + 16);
                std::vector<double> t((size_t)n);
                CHECK(f110_host_map_table(k.data(), H, W, res, kind, pad, t.data(), n, meta) == n);
                const int P = kind == 1 ? pad : 0;
                CHECK(t[(size_t)meta[2] / 8] == 0.0);
                for (int r = 0; r < H; ++r)
                    for (int c = 0; c < W; ++c)
                        CHECK(t[(size_t)(r + P) * meta[1] + c + P] == res * std::sqrt((double)k[(size_t)r * W + c]));
                CHECK(t[(size_t)meta[0] * meta[1] - 1] == res * std::sqrt((double)k[(size_t)H * W - 1]));  // padding: dt[-1,-1]
            }
    }
    std::vector<uint8_t> all_free(12, 1);
    std::vector<uint32_t> k(12);
    CHECK(f110_edt_k(all_free.data(), 3, 4, k.data()) < 0);  // no occupied cell
}

// ---- lookup tables and beam indices --------------------------------------------
static void check_tables() {
    f110_params p;
    f110_default_params(&p);
    for (int td : {2, 3, 2000})
        for (int nb : {2, 3, 63, 1080}) {
            std::vector<double> s(td), c(td), an(nb), bc(nb), sd(nb);
            f110_host_tables(td, nb, 4.7, &p, s.data(), c.data(), an.data(), bc.data(), sd.data());
            CHECK(s[0] == 0.0 && c[0] == 1.0 && an[0] == -4.7 / 2 && sd[nb - 1] > 0.0);
            f110_host_tables(td, nb, 4.7, &p, nullptr, nullptr, nullptr, nullptr, nullptr);
        }
    for (double fov : {0.05, 6.2})
        for (double yaw : {0.0, -3.1, 3.1, 100.0})
            for (int nb : {2, 63, 1080}) {
                std::vector<double> idx(nb);
                const int n = f110_host_beam_indices(yaw, fov, 2000, nb, idx.data());
                CHECK(n >= 1);
                for (double v : idx) CHECK(v >= 0.0 && v < 2000.0);
                CHECK(f110_host_beam_runs_agree(yaw, fov, 2000, nb) >= 0);
            }
    int32_t ranges[4];
    f110_host_window_ranges(0.3, 4.7, 1080, 1.0, 0.2, ranges);
    const double x[3] = {0.0, 1e6, -0.75};
    double sn[3], cs[3];
    uint8_t ok[3], ok2[3];
    f110_host_sincos(x, 3, sn, cs);
    CHECK(sn[0] == 0.0 && cs[0] == 1.0);
    f110_host_sincos_fast(x, 3, sn, cs, ok);
    f110_host_sincos_series(x, 3, sn, cs);
    f110_host_tan_cos_fast(x, 3, sn, cs, ok, ok2);
    const float xf[2] = {0.0f, 2.5f};
    float of[2];
    f110_host_np_sincosf(xf, 2, 1, of);
    CHECK(of[0] == 1.0f);
}

static void check_cell_index() {
    const int H = 5, W = 3;
    const double res = 0.5;
    for (double yaw : {0.0, 0.3}) {
        const double origin[3] = {-1.0, -2.0, yaw};
        std::vector<double> xy;
        for (int r = -1; r <= H; ++r)  // cell centres, the edges themselves and a ring outside the map
            for (int c = -1; c <= W; ++c)
                for (double off : {0.0, 0.5, 1.0}) {
                    const double u = (c + off) * res, v = (r + off) * res;
                    xy.push_back(origin[0] + u * std::cos(yaw) - v * std::sin(yaw));
                    xy.push_back(origin[1] + u * std::sin(yaw) + v * std::cos(yaw));
                }
        const int64_t n = (int64_t)xy.size() / 2;
        std::vector<int64_t> lin((size_t)3 * n);
        CHECK(f110_host_cell_index(H, W, res, origin, xy.data(), n, lin.data()) == F110_OK);
        int64_t i = 0;
        for (int r = -1; r <= H; ++r)
            for (int c = -1; c <= W; ++c)
                for (int o = 0; o < 3; ++o, ++i)
                    if (o == 1 && r >= 0 && r < H && c >= 0 && c < W)  // a cell centre on the map
                        CHECK(lin[3 * i] == r * W + c && lin[3 * i + 1] == r * W + c && lin[3 * i + 2] == r * W + c);
    }
    const double origin[3] = {0, 0, 0};
    CHECK(f110_host_cell_index(0, W, res, origin, nullptr, 0, nullptr) < 0);
}

// ---- the ray launch: plan_ray_launch and ray_rules over their knobs -------------
static void check_ray_plan() {
    const int shape[4][3] = {{1, 1, 2}, {3, 2, 64}, {5, 1, 1080}, {7, 8, 65}};  // E, A, B
    long plans = 0;
    for (int kernel = 1; kernel <= 3; ++kernel)
        for (int lanes = 1; lanes <= 2; ++lanes)
            for (int refill : {0, 1, 3, 16})
                for (int bits = 0; bits < (1 << 11); ++bits)
                    for (const auto &s : shape)
                        for (int theta : {2000, 4096})
                            for (int wpb : {1, 4})
                                for (int masked = 0; masked < 2; ++masked) {
                                    f110_ray_knobs k{};
                                    k.kernel = kernel;
                                    k.lanes = lanes;
                                    k.refill = refill;
                                    k.fxs_lds = bits & 1;
                                    k.count_slots = (bits >> 1) & 1;
                                    k.wtrace = (bits >> 2) & 1;
                                    k.heavy_list = (bits >> 3) & 1;
                                    k.heavy_on = (bits >> 4) & 1;
                                    k.heavy_use = (bits >> 5) & 1;
                                    k.heavy_cap = 64;
                                    k.has_rm = (bits >> 6) & 1;
                                    k.has_rmp = (bits >> 7) & 1;
                                    k.fxs_ok = (bits >> 8) & 1;
                                    k.rotated = (bits >> 9) & 1;
                                    k.has_geo = (bits >> 10) & 1;
                                    k.E = s[0];
                                    k.A = s[1];
                                    k.B = s[2];
                                    k.theta_dis = theta;
                                    k.ray_wpb = wpb;
                                    f110_ray_plan p{};
                                    if (f110_host_ray_plan(&k, masked, &p) != F110_OK || p.grid == 0 || p.block == 0 ||
                                        p.block % 64 != 0 || p.block > 1024 || p.family < F110_RAY_TILED_FLAT ||
                                        p.family > F110_RAY_FXS || (p.family == F110_RAY_FXS && masked))
                                        CHECK(!"plan_ray_launch: a plan out of range");
                                    ++plans;
                                }
    ++g_checks;
    std::printf("ray plans checked: %ld\n", plans);
    f110_ray_knobs bad{};
    f110_ray_plan p{};
    CHECK(f110_host_ray_plan(&bad, 0, &p) < 0);
    for (int64_t own : {1, 4096, 8193, 12288, 16384, 32768, 65536})
        for (int share : {1, 2, 4})
            for (int contexts : {1, 2, 4})
                for (int kernel = 1; kernel <= 3; ++kernel)
                    for (int pad = 0; pad < 2; ++pad) {
                        int32_t r[4] = {-1, -1, -1, -1};
                        CHECK(f110_host_ray_rules(own, own * share, contexts, kernel, pad, r) == F110_OK);
                        CHECK((r[0] == 1 || r[0] == 2) && r[1] >= 0 && r[1] <= 3 && (r[2] | 1) == 1 && (r[3] | 1) == 1);
                        CHECK(kernel == 3 || (r[0] == 1 && r[1] == 0 && r[3] == 0));
                    }
    int32_t r[4];
    CHECK(f110_host_ray_rules(2, 1, 1, 3, 1, r) < 0);
}

// ---- the argument checks of the params and episode-limit setters ------------------
static void check_params() {
    f110_params d;
    f110_default_params(&d);
    const f110_params agents[2] = {d, d};
    f110_params lo[2] = {d, d}, hi[2] = {d, d};
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) == F110_OK);
    lo[1].mu = 0.5;
    hi[1].mu = 1.5;
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) == F110_OK);
    f110_params out;
    CHECK(f110_host_param_draw(7, 3, 1, 2, &lo[1], &hi[1], &out) == F110_OK);
    CHECK(out.mu >= 0.5 && out.mu <= 1.5 && out.m == d.m && out.width == d.width);
    CHECK(f110_host_param_draw(7, 3, 8, 2, &lo[1], &hi[1], &out) < 0);
    lo[1].mu = std::nan("");
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) < 0);
    lo[1].mu = 2.0;  // inverted
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) < 0);
    lo[1].mu = -1e308;  // hi - lo overflows
    hi[1].mu = 1e308;
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) < 0);
    lo[1].mu = hi[1].mu = d.mu;
    hi[0].width = 0.4;  // the car box may not vary
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) < 0);
    hi[0].width = INFINITY;
    CHECK(f110_host_check_param_ranges(lo, hi, agents, 2) < 0);
    CHECK(f110_host_check_param_ranges(nullptr, hi, agents, 2) < 0);
    CHECK(f110_host_check_param_ranges(lo, lo, agents, 0) < 0);
    CHECK(f110_host_check_episode_limits(0, 0.0, 0) == F110_OK);
    CHECK(f110_host_check_episode_limits(100, 0.1, 5) == F110_OK);
    CHECK(f110_host_check_episode_limits(-1, 0.1, 5) < 0);
    CHECK(f110_host_check_episode_limits(1, -0.1, 5) < 0);
    CHECK(f110_host_check_episode_limits(1, std::nan(""), 5) < 0);
    CHECK(f110_host_check_episode_limits(1, 0.1, -5) < 0);
    CHECK(f110_last_error()[0] != 0);
}

// ---- the n-step host model ---------------------------------------------------------
static void check_nstep() {
    const int64_t N = 3;
    const int D = 3, A = 2;
    for (int n : {1, 16}) {
        std::vector<int32_t> len(N, 0), head(N, 0), k((size_t)N * n, 0);
        std::vector<double> ret((size_t)N * n, 0.0), reward(N);
        std::vector<float> win_obs((size_t)N * n * D, 0.f), win_act((size_t)N * n * A, 0.f), obs((size_t)N * D),
            act((size_t)N * A), next_obs((size_t)N * D);
        std::vector<uint8_t> term(N), trunc(N), was_reset(N);
        std::vector<float> out_obs((size_t)N * n * D), out_act((size_t)N * n * A), out_reward((size_t)N * n),
            out_next((size_t)N * n * D), out_done((size_t)N * n);
        int64_t total = 0, transitions = 0;
        for (int t = 0; t < 40; ++t) {
            for (int64_t e = 0; e < N; ++e) {
                reward[e] = 1.0 + e;
                was_reset[e] = t > 0 && (term[e] || trunc[e]);  // the row after an episode's end is its reset
                term[e] = !was_reset[e] && (t + e) % 11 == 10;
                trunc[e] = !was_reset[e] && (t + 2 * e) % 17 == 16;
                transitions += !was_reset[e];
                for (int j = 0; j < D; ++j) obs[e * D + j] = (float)t, next_obs[e * D + j] = (float)(t + 1);
                for (int j = 0; j < A; ++j) act[e * A + j] = (float)(t * 10 + e);
            }
            int64_t count = -1;
            CHECK(f110_host_nstep(N, n, 0.99, D, A, N * n, len.data(), head.data(), ret.data(), k.data(),
                                  win_obs.data(), win_act.data(), obs.data(), act.data(), reward.data(),
                                  next_obs.data(), term.data(), t % 2 ? trunc.data() : nullptr, was_reset.data(),
                                  out_obs.data(), out_act.data(), out_reward.data(), out_next.data(),
                                  out_done.data(), &count) == F110_OK);
            CHECK(count >= 0 && count <= N * n);
            for (int64_t e = 0; e < N; ++e) CHECK(len[e] >= 0 && len[e] <= n && head[e] >= 0 && head[e] < n);
            total += count;
        }
        CHECK(total > 0 && total <= transitions);
        if (n == 1) CHECK(total == transitions);  // a 1-step window emits every transition at once
        int64_t count = 0;
        CHECK(f110_host_nstep(N, n, 0.99, D, A, N * n - 1, len.data(), head.data(), ret.data(), k.data(),
                              win_obs.data(), win_act.data(), obs.data(), act.data(), reward.data(), next_obs.data(),
                              term.data(), nullptr, was_reset.data(), out_obs.data(), out_act.data(),
                              out_reward.data(), out_next.data(), out_done.data(), &count) < 0);  // capacity
    }
    int64_t count = 0;
    CHECK(f110_host_nstep(N, 17, 0.99, D, A, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          &count) < 0);
}

// ---- episode statistics ----------------------------------------------------------
static void check_episode_stats() {
    for (int64_t E : {0, 1, 257}) {
        const size_t n = (size_t)E;
        std::vector<double> rewards(n, 0.5), last_return(n, -1.0);
        std::vector<uint8_t> term(n, 0), trunc(n, 0), was_reset(n, 0), finished(n, 9);
        std::vector<int32_t> last_length(n, -1);
        std::vector<f110_episode_state> state(n);
        for (auto &s : state) s = f110_episode_state{};
        f110_episode_totals totals{};
        // (data() of an empty vector may be null: the checks want non-null pointers also at 0 envs)
        double r0 = 0;
        uint8_t b0 = 0;
        f110_episode_state s0{};
        for (int t = 0; t < 5; ++t) {
            for (size_t e = 0; e < n; ++e) {
                was_reset[e] = t > 0 && (term[e] || trunc[e]);  // the row after an episode's end is its reset
                term[e] = !was_reset[e] && (t + e) % 3 == 2;
                trunc[e] = !was_reset[e] && (t + e) % 5 == 4;
            }
            CHECK(f110_host_episode_stats(n ? rewards.data() : &r0, n ? term.data() : &b0, t % 2 ? nullptr : (n ? trunc.data() : &b0),
                                          n ? was_reset.data() : &b0, E, n ? state.data() : &s0,
                                          t == 4 ? nullptr : last_return.data(), last_length.data(), finished.data(),
                                          &totals) == F110_OK);
            for (size_t e = 0; e < n; ++e) CHECK(finished[e] <= 1);
        }
        CHECK(totals.episodes >= 0 && totals.episodes <= 5 * E && totals.terminated + totals.truncated == totals.episodes);
        CHECK(E == 0 ? totals.episodes == 0 : totals.episodes > 0);
        CHECK(f110_host_episode_stats(nullptr, &b0, nullptr, &b0, E, &s0, nullptr, nullptr, nullptr, &totals) < 0);
    }
}

// ---- a track's derived arrays and midpoint grid ----------------------------------
static void check_track() {
    for (int n : {2, 3, 50}) {
        std::vector<double> xy((size_t)2 * n), s, tan, nrm, mid;
        for (int i = 0; i < n; ++i) xy[2 * i] = 5.0 * std::cos(0.1 * i), xy[2 * i + 1] = 5.0 * std::sin(0.1 * i);
        track_arrays(xy.data(), n, s, tan, nrm, mid);
        CHECK(s.size() == (size_t)n && tan.size() == (size_t)2 * (n - 1) && mid.size() == tan.size() && s[n - 1] > 0.0);
        const TrackGrid g = track_grid(xy.data(), n, mid);
        CHECK(!g.cstart.empty() && g.cstart.size() == (size_t)g.gnx * g.gny + 1 && g.cstart.back() == n - 1);
        CHECK(g.citems.size() == (size_t)n - 1 && g.cmid.size() == (size_t)2 * (n - 1));
    }
    const double same[4] = {1.0, 1.0, 1.0, 1.0};  // a degenerate centerline: no grid, no stray index
    std::vector<double> s, tan, nrm, mid;
    track_arrays(same, 2, s, tan, nrm, mid);
    CHECK(track_grid(same, 2, mid).cstart.empty());
}

int main() {
    CHECK(f110_abi_version() == F110_ABI_VERSION);
    check_maps();
    check_tables();
    check_cell_index();
    check_ray_plan();
    check_params();
    check_nstep();
    check_episode_stats();
    check_track();
    std::printf("host_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
