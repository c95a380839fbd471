// track_obs_check.cpp — a stand-alone program over the track observation's row rule
// (csrc/f110_track_obs.h), to be built with AddressSanitizer and UBSan on the CPU
// (scripts/host_check.sh), in the manner of host_check.cpp.  f110_host_track_obs itself sits beside
// the launchers (csrc/f110_task_capi.cpp) and cannot be linked without the device code; its
// arithmetic and its argument check are this header's, run here on a track's derived arrays
// (csrc/f110_host.cpp) of exactly the documented lengths, with the last segment, the last node and
// the state's last column used.  Not a pytest test; it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_host.h"
#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_sincos.h"
#include "../../f110_gymnasium_ros2_jazzy_amd/csrc/f110_track_obs.h"
#include "../../include/f110.h"

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

// ---- the track observation's row rule (csrc/f110_track_obs.h) ---------------------
static void check_track_obs() {
    const int n = 6;
    std::vector<double> xy((size_t)2 * n), s, tan, nrm, mid;
    for (int i = 0; i < n; ++i) xy[2 * i] = 2.0 * i, xy[2 * i + 1] = 0.25 * i * i;
    track_arrays(xy.data(), n, s, tan, nrm, mid);
    const double L = s[n - 1];
    f110_track_obs_params P{};
    P.v_scale = 20.0, P.steer_scale = 0.4189, P.yaw_rate_scale = 10.0, P.slip_scale = 1.0, P.lat_scale = 1.0;
    P.gap_scale = 10.0, P.n_preview = 8, P.direction = 1;
    for (int j = 0; j < 8; ++j) P.preview[j] = 0.5 * (j + 1);
    CHECK(track_obs_width(0, 0) == 8 && track_obs_width(4, 1) == 20 && track_obs_width(8, 1) == kTrackObsMaxWidth);
    for (int A = 1; A <= 3; ++A) {
        const int64_t E = 3, EA = E * A;
        std::vector<double> state((size_t)7 * EA);
        for (size_t i = 0; i < state.size(); ++i) state[i] = 0.37 * (double)(i % 11) - 1.0;
        std::vector<float> out((size_t)E * kTrackObsMaxWidth);
        const int other = A > 1 ? A - 1 : -1;
        CHECK(!track_obs_bad_args(&P, L, state.data(), E, A, 0, other, out.data(), track_obs_width(8, other >= 0)));
        CHECK(track_obs_bad_args(&P, L, state.data(), E, A, 0, other, out.data(), track_obs_width(8, other >= 0) - 1));
        CHECK(track_obs_bad_args(&P, L, state.data(), E, A, A, other, out.data(), 64));
        CHECK(track_obs_bad_args(&P, L, state.data(), E, A, 0, 0, out.data(), 64));
        for (int64_t e = 0; e < E; ++e)
            for (int dir = -1; dir <= 1; dir += 2) {
                P.direction = dir;
                const TrackObsCar c = track_obs_car(state.data(), EA, e * A + (A - 1));  // the state's last column too
                double sn, cs, own[kTrackObsOwn], gap[kTrackObsGap];
                cr_sincos(c.yaw, sn, cs);
                track_obs_own(P, c, 0.3, tan[2 * (n - 2)], tan[2 * (n - 2) + 1], sn, cs, own);
                CHECK(std::fabs(own[5] * own[5] + own[6] * own[6] - 1.0) < 1e-12);
                for (int closed = 0; closed <= 1; ++closed)
                    for (double s_p : {0.0, 0.4 * L, L}) {
                        for (int j = 0; j < P.n_preview; ++j) {
                            const double sq = track_obs_query(P, P.preview[j], s_p, closed, L);
                            CHECK(sq >= 0.0 && sq <= L);
                            int k = n - 2;  // searchsorted(s, sq, "right") - 1 clipped to [0, n-2]
                            while (k > 0 && s[k] > sq) --k;
                            double px, py;
                            track_obs_preview(xy.data(), s.data(), k, sq, P.preview[j], c.x, c.y, sn, cs, px, py);
                            CHECK(std::isfinite(px) && std::isfinite(py));
                        }
                        track_obs_gap(P, closed, L, s_p, 0.3, c.v, 0.9 * L, -0.2, 1.0, gap);
                        CHECK(gap[0] >= -1.0 && gap[0] <= 1.0 && std::isfinite(gap[1]) && std::isfinite(gap[2]));
                    }
            }
        P.direction = 1;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double st[7] = {0};
    float o[kTrackObsMaxWidth];
    f110_track_obs_params Q = P;
    Q.gap_scale = nan;
    CHECK(track_obs_bad_args(&Q, L, st, 1, 1, 0, -1, o, 64));
    Q = P;
    Q.preview[7] = L;
    CHECK(track_obs_bad_args(&Q, L, st, 1, 1, 0, -1, o, 64));
    Q.n_preview = 7;  // an unused distance is not looked at
    CHECK(!track_obs_bad_args(&Q, L, st, 1, 1, 0, -1, o, 64));
    Q.n_preview = 9;
    CHECK(track_obs_bad_args(&Q, L, st, 1, 1, 0, -1, o, 64));
    CHECK(track_obs_bad_args(nullptr, L, st, 1, 1, 0, -1, o, 64));
}

int main() {
    check_track_obs();
    std::printf("track_obs_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
