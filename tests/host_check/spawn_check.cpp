// spawn_check.cpp — a stand-alone program over the spawn randomization's host statement
// (f110_host_spawn_rows, csrc/f110_host.cpp; the row rule: csrc/f110_spawn.h), to be built with
// AddressSanitizer and UBSan on the CPU (scripts/host_check.sh), in the manner of host_check.cpp.
// Every array has exactly the documented length, so a lookup one cell past the EDT, a read past the
// spawn table's last row or a write past the output is reported: the clearance fallback through
// all five outcomes, the gap's wrap at both table ends (rows 0 and n - 1, magnitudes beyond n), and
// base poses outside the map, at NaN and at +-inf, whose lookups must land on the last cell.
// Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_spawn.h"
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

// a box of H x W cells with walls on its border: the EDT is the distance to the nearest border cell
static const int32_t H = 20, W = 40;
static const double RES = 0.1, ORIGIN[3] = {0.0, 0.0, 0.0};

static std::vector<double> box_edt() {
    std::vector<double> d((size_t)H * W);  // exactly H * W: no slack behind the last cell
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            int m = r < H - 1 - r ? r : H - 1 - r;
            m = c < m ? c : m;
            m = W - 1 - c < m ? W - 1 - c : m;
            d[(size_t)r * W + c] = RES * m;
        }
    return d;
}

static f110_spawn_range range(double lat_lo, double lat_hi, int32_t gap_lo, int32_t gap_hi, double behind,
                              double clearance) {
    f110_spawn_range r{};
    r.lateral[0] = lat_lo;
    r.lateral[1] = lat_hi;
    r.heading[0] = -0.2;
    r.heading[1] = 0.2;
    r.speed[0] = 1.0;
    r.speed[1] = 6.0;
    r.gap[0] = gap_lo;
    r.gap[1] = gap_hi;
    r.behind = behind;
    r.clearance = clearance;
    return r;
}

static void clearance_fallback(const std::vector<double> &edt) {
    // base poses along y = 1.0 (the box's middle row), yaw 0: the offset runs along +y towards the
    // wall at y = 2.0, then beyond the map (d up to 8 m: d / 8 can still fail, the fifth outcome)
    const int64_t n = 512;
    const f110_spawn_range r = range(0.0, 8.0, 0, 0, 0.0, 0.35);
    std::vector<double> poses((size_t)n * 3), out((size_t)n * 4);
    std::vector<int64_t> envs((size_t)n);
    std::vector<int32_t> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        envs[(size_t)i] = i;
        poses[(size_t)i * 3] = 2.0;
        poses[(size_t)i * 3 + 1] = 1.0;
        poses[(size_t)i * 3 + 2] = 0.0;
    }
    CHECK(f110_host_spawn_rows(&r, 1, 5, 0, edt.data(), H, W, RES, ORIGIN, nullptr, 0, poses.data(), nullptr,
                               envs.data(), nullptr, n, 0, out.data(), rows.data()) == F110_OK);
    const MapView m{edt.data(), H, W, (int64_t)H * W, RES, 0.0, 0.0, 1.0, 0.0, W * RES, H * RES, 1.0 / RES};
    int taken[5] = {0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const SpawnDraws w = spawn_draws(5, (uint64_t)i, 0, 0, r);
        const double t[5] = {w.d, w.d * 0.5, w.d * 0.25, w.d * 0.125, 0.0};
        int first = 4;
        for (int k = 3; k >= 0; --k)
            if (edt[(size_t)cell_index(m, 2.0, 1.0 + t[k])] >= 0.35) first = k;
        ++taken[first];
        CHECK(out[(size_t)i * 4] == 2.0 && out[(size_t)i * 4 + 1] == 1.0 + t[first]);
        CHECK(out[(size_t)i * 4 + 2] == w.dth && out[(size_t)i * 4 + 3] == w.v0);  // never adjusted
        CHECK(rows[(size_t)i] == -1);
    }
    for (int k = 0; k < 5; ++k) CHECK(taken[k] > 0);
}

static void gap_wrap(const std::vector<double> &edt) {
    const int32_t n_spawn = 7, A = 2;
    std::vector<double> spawn((size_t)n_spawn * A * 3);  // exactly the table: a row past either end is reported
    for (int k = 0; k < n_spawn; ++k)
        for (int a = 0; a < A; ++a) {
            double *p = &spawn[((size_t)k * A + a) * 3];
            p[0] = 1.0 + 0.2 * k;
            p[1] = 0.8 + 0.4 * a;
            p[2] = 0.0;
        }
    const int32_t mags[5] = {1, 6, 7, 20, 2147483647};
    for (int32_t mag : mags)
        for (int behind = 0; behind < 2; ++behind) {
            const f110_spawn_range r[2] = {range(0.0, 0.0, 0, 0, 0.0, 0.0), range(0.0, 0.0, mag, mag, behind, 0.0)};
            std::vector<int32_t> k((size_t)n_spawn), rows((size_t)n_spawn * A);
            std::vector<int64_t> envs((size_t)n_spawn);
            std::vector<uint64_t> ep((size_t)n_spawn, 1);
            std::vector<double> out((size_t)n_spawn * A * 4);
            for (int i = 0; i < n_spawn; ++i) {
                k[(size_t)i] = i;
                envs[(size_t)i] = 100 + i;
            }
            CHECK(f110_host_spawn_rows(r, A, 9, 0, edt.data(), H, W, RES, ORIGIN, spawn.data(), n_spawn, nullptr, k.data(),
                                       envs.data(), ep.data(), n_spawn, 0, out.data(), rows.data()) == F110_OK);
            for (int i = 0; i < n_spawn; ++i) {
                const int64_t want = behind ? ((i - (int64_t)mag) % n_spawn + n_spawn) % n_spawn : (i + (int64_t)mag) % n_spawn;
                CHECK(rows[(size_t)i * A] == i && rows[(size_t)i * A + 1] == want);
                CHECK(out[((size_t)i * A + 1) * 4] == spawn[(size_t)want * A * 3]);        // column 0 of that row
                CHECK(out[((size_t)i * A + 1) * 4 + 1] == spawn[(size_t)want * A * 3 + 1]);
                CHECK(out[((size_t)i * A) * 4 + 1] == 0.8);                                // the ego: its own column
            }
            // the context's own row draw (rows == NULL): inside the table
            CHECK(f110_host_spawn_rows(r, A, 9, 77, edt.data(), H, W, RES, ORIGIN, spawn.data(), n_spawn, nullptr, nullptr,
                                       envs.data(), ep.data(), n_spawn, 1, out.data(), rows.data()) == F110_OK);
            for (int32_t v : rows) CHECK(v >= 0 && v < n_spawn);
        }
    // refused before anything is read: a row outside the table, an autoreset without a table or an episode
    const f110_spawn_range r[2] = {range(0.0, 0.0, 0, 0, 0.0, 0.0), range(0.0, 0.0, 1, 2, 0.5, 0.0)};
    const int32_t bad_row = n_spawn;
    const int64_t env = 0;
    const uint64_t ep1 = 1, ep0 = 0;
    double out[8];
    CHECK(f110_host_spawn_rows(r, A, 9, 0, edt.data(), H, W, RES, ORIGIN, spawn.data(), n_spawn, nullptr, &bad_row, &env,
                               &ep1, 1, 0, out, nullptr) == F110_E_INVALID);
    CHECK(f110_host_spawn_rows(r, A, 9, 0, edt.data(), H, W, RES, ORIGIN, nullptr, 0, nullptr, nullptr, &env, &ep1, 1, 0, out,
                               nullptr) == F110_E_INVALID);
    CHECK(f110_host_spawn_rows(r, A, 9, 0, edt.data(), H, W, RES, ORIGIN, spawn.data(), n_spawn, nullptr, nullptr, &env,
                               &ep0, 1, 0, out, nullptr) == F110_E_INVALID);
    CHECK(f110_host_check_spawn_ranges(r, A, 0) == F110_E_INVALID);  // a gap without a table
    CHECK(f110_host_check_spawn_ranges(r, A, n_spawn) == F110_OK);
}

static void out_of_map(const std::vector<double> &edt) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bases[8][3] = {{-5.0, 1.0, 0.0},  {50.0, 1.0, 1.0}, {2.0, -3.0, 2.0},   {2.0, 1e30, 0.5},
                                {inf, 1.0, 0.0},   {2.0, -inf, 0.0}, {nan, nan, 0.0},    {2.0, 1.0, nan}};
    const int64_t n = 8;
    const f110_spawn_range r = range(-1e6, 1e6, 0, 0, 0.0, 0.05);
    std::vector<double> poses((size_t)n * 3), out((size_t)n * 4);
    std::vector<int64_t> envs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        envs[(size_t)i] = (int64_t)1 << (4 * i);
        for (int k = 0; k < 3; ++k) poses[(size_t)i * 3 + k] = bases[i][k];
    }
    for (int f32 = 0; f32 < 2; ++f32) {
        CHECK(f110_host_spawn_rows(&r, 1, 1, 0, edt.data(), H, W, RES, ORIGIN, nullptr, 0, poses.data(), nullptr,
                                   envs.data(), nullptr, n, f32, out.data(), nullptr) == F110_OK);
        // the last cell is a wall cell (0 < clearance): every off-map try is refused, so d = 0 and the
        // finite bases come back as they went in (float32-rounded under f32)
        for (int64_t i = 0; i < 4; ++i) {
            const double x = bases[i][0], y = bases[i][1];
            CHECK(out[(size_t)i * 4] == (f32 ? (double)(float)x : x));
            CHECK(out[(size_t)i * 4 + 1] == (f32 ? (double)(float)y : y));
        }
        for (int64_t i = 0; i < n; ++i) CHECK(out[(size_t)i * 4 + 3] >= 1.0 && out[(size_t)i * 4 + 3] < 6.0);
    }
}

int main() {
    const std::vector<double> edt = box_edt();
    clearance_fallback(edt);
    gap_wrap(edt);
    out_of_map(edt);
    std::printf("spawn_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
