// f110_host.cpp — the pure host code of libf110.so: everything that makes no HIP runtime call and
// touches no handle.  The error string, the defaults, the reference's lookup tables, the exact EDT
// (Felzenszwalb-Huttenlocher lower envelopes, integer arithmetic) and the tables built from it,
// the beam-index and sin/cos test hooks, the ray-launch decision (ray_rules, plan_ray_launch), the
// argument checks of the params / episode / n-step entry points and their host models, the
// derivation of a track's arrays, and the host statements of the scan observation, the spawn
// randomization and the sensor randomization.  It links on its own (tests/host_check runs it under ASan / UBSan).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_beam_runs.h"
#include "f110_env_rows.h"
#include "f110_geometry.h"
#include "f110_host.h"
#include "f110_host_util.h"
#include "f110_learner_args.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_scan_obs.h"
#include "f110_sensor.h"
#include "f110_sincos.h"
#include "f110_spawn.h"
#include "f110_step_args.h"
#include "f110_task_args.h"

using namespace f110;

// ---------------------------------------------------------------- misc ----
namespace {
thread_local std::string g_err;
}  // namespace

int f110_set_error(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

extern "C" int f110_abi_version(void) { return F110_ABI_VERSION; }
extern "C" const char *f110_last_error(void) { return g_err.c_str(); }

extern "C" void f110_default_params(f110_params *p) {
    // f110_env.py:132-156
    p->mu = 1.0489;
    p->C_Sf = 4.718;
    p->C_Sr = 5.4562;
    p->lf = 0.15875;
    p->lr = 0.17145;
    p->h = 0.074;
    p->m = 3.74;
    p->I = 0.04712;
    p->s_min = -0.4189;
    p->s_max = 0.4189;
    p->sv_min = -3.2;
    p->sv_max = 3.2;
    p->v_switch = 7.319;
    p->a_max = 9.51;
    p->v_min = 0.00000001;
    p->v_max = 20.0;
    p->width = 0.31;
    p->length = 0.58;
    p->lidar_max = 30.0;
}

extern "C" void f110_default_config(f110_config *c) {
    std::memset(c, 0, sizeof(*c));
    c->n_envs = 1;
    c->n_agents = 2;            // f110_env.py:159-162
    c->n_beams = 1080;          // base_classes.py:69
    c->theta_dis = 2000;        // laser_models.py:360
    c->integrator = F110_INTEGRATOR_RK4;  // f110_env.py:176-179
    c->ego_idx = 0;
    c->autoreset = 0;
    c->fov = 4.7;
    c->eps = 0.0001;
    c->max_range = 30.0;
    c->time_step = 0.01;
    c->lidar_dist = 0.0;
    c->ttc_thresh = 0.005;
    c->noise_std = 0.01;
    c->env_offset = 0;
    c->seed = 42;               // f110_env.py:110-113
}

extern "C" void f110_default_reward_params(f110_reward_params *p) {
    if (!p) return;
    *p = f110_reward_params{};
    // CenterlineSafetyProgressReward.__init__ defaults (rewards.py:196-230)
    p->dt = 0.01;
    p->w_prog = 1.2;
    p->forward_sign = 1.0;
    p->alive_bonus = 0.02;
    p->w_rel_lead = 0.0;
    p->lead_clip = 5.0;
    p->w_lat = 0.35;
    p->lat_cap = 4.0;
    p->default_half_width = 1.5;
    p->lidar_max = 1.0;  // LIDAR_MAX (rewards.py:7)
    p->near_wall_dist = 0.35 / 30.0;
    p->w_wall = 1.0;
    p->wall_quantile = 0.05;
    p->opp_safe_dist = 0.7;
    p->w_opp = 0.8;
    p->ego_crash_penalty = 50.0;
    p->opp_crash_bonus = 50.0;
    p->beta = 0.8;
    p->grace_steps_wall = 25;
    p->grace_steps_opp = 25;
    p->auto_flip_steps = 20;
    p->use_progress = 1;
}

// ----------------------------------------------------------------- tables --
// Host computation of the reference's lookup tables, exactly as NumPy does it
// (each sin/cos called separately: glibc sincos() differs in the last bit).
static double (*volatile g_sin)(double) = ::sin;  // volatile: keep sin/cos separate calls
static double (*volatile g_cos)(double) = ::cos;

extern "C" void f110_host_tables(int32_t theta_dis, int32_t n_beams, double fov, const f110_params *p, double *sines,
                      double *cosines, double *angles, double *beam_cos, double *side) {
    // ScanSimulator2D.__init__, laser_models.py:379-381: linspace(0, 2pi, theta_dis)
    const double stop = 2.0 * kPi;
    const double step = stop / (double)(theta_dis - 1);
    for (int i = 0; i < theta_dis; ++i) {
        double th = (i == theta_dis - 1) ? stop : (double)i * step;
        if (sines) sines[i] = g_sin(th);
        if (cosines) cosines[i] = g_cos(th);
    }
    // RaceCar.__init__, base_classes.py:122-158
    const double incr = fov / (double)(n_beams - 1);
    const double dist_sides = p->width / 2.;
    const double dist_fr = (p->lf + p->lr) / 2.;
    for (int i = 0; i < n_beams; ++i) {
        double angle = -fov / 2. + (double)i * incr;
        if (angles) angles[i] = angle;
        if (beam_cos) beam_cos[i] = g_cos(angle);
        double to_side, to_fr;
        if (angle > 0) {
            if (angle < kPi / 2) {
                to_side = dist_sides / g_sin(angle);
                to_fr = dist_fr / g_cos(angle);
            } else {
                to_side = dist_sides / g_cos(angle - kPi / 2.);
                to_fr = dist_fr / g_sin(angle - kPi / 2.);
            }
        } else {
            if (angle > -kPi / 2) {
                to_side = dist_sides / g_sin(-angle);
                to_fr = dist_fr / g_cos(-angle);
            } else {
                to_side = dist_sides / g_cos(-angle - kPi / 2);
                to_fr = dist_fr / g_sin(-angle - kPi / 2);
            }
        }
        if (side) side[i] = to_fr < to_side ? to_fr : to_side;  // Python min()
    }
}

// Host evaluation of the beam-index runs (tests the run construction on CPU).
extern "C" int f110_host_beam_indices(double yaw, double fov, int32_t theta_dis, int32_t n_beams,
                                      double *theta_index_out) {
    const double inc = (double)theta_dis * (fov / (double)(n_beams - 1)) / (2. * kPi);
    BeamRun runs[kMaxSeg];
    double t0 = first_theta_index(yaw, fov, theta_dis);
    int n = build_beam_runs(t0, inc, theta_dis, n_beams, runs, kMaxSeg);
    if (n < 0) return fail(F110_E_INVALID, "beam index runs exceed kMaxSeg");
    for (int b = 0; b < n_beams; ++b) theta_index_out[b] = beam_theta_index(runs, n, b);
    return n;
}

// The two run builders against each other at yaw (k_agents uses build_beam_runs_fast): 1 when
// they give the same runs, 0 when not, < 0 on error.
extern "C" int f110_host_beam_runs_agree(double yaw, double fov, int32_t theta_dis, int32_t n_beams) {
    const double inc = (double)theta_dis * (fov / (double)(n_beams - 1)) / (2. * kPi);
    BeamRun r0[kMaxSeg], r1[kMaxSeg];
    const double t0 = first_theta_index(yaw, fov, theta_dis);
    const int n0 = build_beam_runs(t0, inc, theta_dis, n_beams, r0, kMaxSeg);
    const int n1 = build_beam_runs_fast(t0, inc, theta_dis, n_beams, r1, kMaxSeg);
    if (n0 != n1) return 0;
    for (int i = 0; i < n0; ++i)
        if (r0[i].start != r1[i].start || r0[i].count != r1[i].count ||
            std::memcmp(&r0[i].t0, &r1[i].t0, 8) != 0 || std::memcmp(&r0[i].delta, &r1[i].delta, 8) != 0)
            return 0;
    return 1;
}

extern "C" void f110_host_sincos(const double *x, int64_t n, double *sn, double *cs) {
    for (int64_t i = 0; i < n; ++i) cr_sincos(x[i], sn[i], cs[i]);
}

extern "C" void f110_host_tan_cos_fast(const double *x, int64_t n, double *t, double *c, uint8_t *ok_t,
                                       uint8_t *ok_c) {
    for (int64_t i = 0; i < n; ++i) {
        bool a, b;
        tan_cos_fast(x[i], kSinCosTab, t[i], c[i], a, b);
        ok_t[i] = a ? 1 : 0;
        ok_c[i] = b ? 1 : 0;
    }
}

extern "C" void f110_host_sincos_fast(const double *x, int64_t n, double *sn, double *cs, uint8_t *ok) {
    for (int64_t i = 0; i < n; ++i) ok[i] = cr_sincos_fast(x[i], sn[i], cs[i]) ? 1 : 0;
}

extern "C" void f110_host_sincos_series(const double *x, int64_t n, double *sn, double *cs) {
    for (int64_t i = 0; i < n; ++i) cr_sincos_series(x[i], sn[i], cs[i]);
}

extern "C" void f110_host_np_sincosf(const float *x, int64_t n, int32_t cos_op, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = np_sincosf(x[i], cos_op != 0);
}

extern "C" void f110_host_window_ranges(double yaw, double fov, int32_t n_beams, double center, double half,
                                        int32_t ranges_out[4]) {
    int r0a, r0b, r1a, r1b;
    window_beam_ranges(yaw, fov, fov / (double)(n_beams - 1), n_beams, center, half, r0a, r0b, r1a, r1b);
    ranges_out[0] = r0a;
    ranges_out[1] = r0b;
    ranges_out[2] = r1a;
    ranges_out[3] = r1b;
}

// ---------------------------------------------------------------- EDT ----
// 1-D lower envelope of parabolas y = (x - q)^2 + f[q] over the finite sites,
// compared as exact rationals (Felzenszwalb & Huttenlocher 2012).
namespace {
constexpr int64_t kInf = INT64_MAX / 4;

void edt_1d(const int64_t *f, int n, int64_t *d, int *v, int64_t *zn, int64_t *zd) {
    int k = -1;
    for (int q = 0; q < n; ++q) {
        if (f[q] >= kInf) continue;
        while (k >= 0) {
            int p = v[k];
            // intersection of parabolas q and p: s = N / D
            int64_t N = (f[q] + (int64_t)q * q) - (f[p] + (int64_t)p * p);
            int64_t D = 2 * (int64_t)(q - p);
            if (k == 0) break;
            // drop p if s(q,p) <= z[k] = zn[k]/zd[k]
            if ((__int128)N * zd[k] <= (__int128)zn[k] * D) {
                --k;
            } else {
                break;
            }
        }
        ++k;
        v[k] = q;
        if (k > 0) {
            int p = v[k - 1];
            zn[k] = (f[q] + (int64_t)q * q) - (f[p] + (int64_t)p * p);
            zd[k] = 2 * (int64_t)(q - p);
        }
    }
    if (k < 0) {
        for (int x = 0; x < n; ++x) d[x] = kInf;
        return;
    }
    int j = 0;
    for (int x = 0; x < n; ++x) {
        // advance while z[j+1] < x
        while (j < k && (__int128)zn[j + 1] < (__int128)x * zd[j + 1]) ++j;
        int64_t dx = x - v[j];
        d[x] = dx * dx + f[v[j]];
    }
}
}  // namespace

extern "C" int f110_edt_k(const uint8_t *free_mask, int32_t H, int32_t W, uint32_t *k_out) {
    if (!free_mask || !k_out || H <= 0 || W <= 0) return fail(F110_E_INVALID, "f110_edt_k: bad arguments");
    const size_t N = (size_t)H * W;
    std::vector<int64_t> g(N);
    bool any = false;
    // pass 1: squared distance along each column to the nearest occupied cell
    std::vector<int64_t> col(H), out(H);
    std::vector<int> v(H > W ? H : W);
    std::vector<int64_t> zn((H > W ? H : W) + 1), zd((H > W ? H : W) + 1);
    for (int c = 0; c < W; ++c) {
        for (int r = 0; r < H; ++r) {
            bool occ = free_mask[(size_t)r * W + c] == 0;
            col[r] = occ ? 0 : kInf;
            any = any || occ;
        }
        edt_1d(col.data(), H, out.data(), v.data(), zn.data(), zd.data());
        for (int r = 0; r < H; ++r) g[(size_t)r * W + c] = out[r];
    }
    if (!any) return fail(F110_E_INVALID, "f110_edt_k: map has no occupied cell (EDT undefined)");
    // pass 2: rows
    std::vector<int64_t> row(W), rout(W);
    for (int r = 0; r < H; ++r) {
        for (int c = 0; c < W; ++c) row[c] = g[(size_t)r * W + c];
        edt_1d(row.data(), W, rout.data(), v.data(), zn.data(), zd.data());
        for (int c = 0; c < W; ++c) {
            if (rout[c] > 0xFFFFFFFFll) return fail(F110_E_INVALID, "f110_edt_k: distance overflows uint32");
            k_out[(size_t)r * W + c] = (uint32_t)rout[c];
        }
    }
    return F110_OK;
}

// ------------------------------------------------- map views and EDT tables --
namespace f110 {

// k_rays_fx's preconditions (f110_rays_fx.h): an axis-aligned map (origin
// yaw 0: cos 1, sin 0 exactly, so x_rot == x_trans), one-wave blocks, H and W
// below 2^21 and |origin / res| below 2^20 (on-map t = 1.5*2^22 + q stays in
// [2^22, 2^23)), and every EDT entry 0 or above eps (the loop's d > eps is
// then d != 0; the smallest non-zero entry is res * sqrt(1)).
bool fx_eligible(int32_t H, int32_t W, double res, const double origin[3], double eps, const uint32_t *edt_k,
                 int32_t wpb) {
    if (origin[2] != 0.0 || wpb != 1) return false;
    if (H >= (1 << 21) || W >= (1 << 19)) return false;  // fx_offset's 24-bit multiply by wt * 128
    const double ir = 1.0 / res;
    if (!(std::fabs(origin[0] * ir) < 1048576.0) || !(std::fabs(origin[1] * ir) < 1048576.0)) return false;
    uint32_t kmin = 0;
    for (size_t i = 0, n = (size_t)H * W; i < n; ++i)
        if (edt_k[i] && (!kmin || edt_k[i] < kmin)) kmin = edt_k[i];
    return !kmin || res * std::sqrt((double)kmin) > eps;
}

// k_rays_fxn / k_rays_fxs's padded table (PAD, see kFxpBase): cell (r, c) at
// row r + P, column c + P; every other cell holds dt[-1,-1] (the reference's
// off-map read), and a 0.0 after the last row is the zero cell.  Rows of Wp =
// 511 mod 512 cells: the row stride Wp * 8 is 8 bytes short of a multiple of
// 4096, which k_rays_fxs's offset arithmetic needs (kFxsBase); any width
// serves the others.  Built only where its byte offsets stay 32-bit and a row
// stride stays a 24-bit multiplier (else empty: the clamped table is used).
std::vector<double> host_padded_table(int32_t H, int32_t W, int32_t pad, const std::vector<double> &d, size_t &Wp,
                                      size_t &Hp) {
    const size_t N = (size_t)H * W, P = (size_t)pad;
    Wp = ((size_t)W + 2 * P + 1 + 511) / 512 * 512 - 1;
    Hp = (size_t)H + 2 * P;
    if (pad <= 0 || d.size() != N || (Wp * Hp + 16) * 8 >= (1ull << 32) || Wp * 8 >= (1u << 24)) return {};
    std::vector<double> rmp(Wp * Hp + 16, d[N - 1]);
    for (size_t r = 0; r < (size_t)H; ++r)
        for (size_t q = 0; q < (size_t)W; ++q) rmp[(r + P) * Wp + q + P] = d[r * W + q];
    rmp[Wp * Hp] = 0.0;
    return rmp;
}

// k_rays_fx / k_rays_fxn's row-major EDT: rows of Wp cells (W + 1 rounded up
// to 16: 128-B aligned), the padding columns and row H hold dt[-1,-1] (a
// clamped index then reads the reference's off-map value), and a 0.0 after
// the last row is the zero cell of rays that have ended.
std::vector<double> host_rowmajor_table(int32_t H, int32_t W, const std::vector<double> &d, size_t &Wp, size_t &Hp) {
    const size_t N = (size_t)H * W;
    Wp = ((size_t)W + 1 + 15) / 16 * 16;
    Hp = (size_t)H + 1;
    if (d.size() != N) return {};
    std::vector<double> rm(Wp * Hp + 16, d[N - 1]);
    for (size_t r = 0; r < (size_t)H; ++r)
        for (size_t q = 0; q < (size_t)W; ++q) rm[r * Wp + q] = d[r * W + q];
    rm[Wp * Hp] = 0.0;
    return rm;
}

// dt = res * EDT (get_dt, laser_models.py:52) -- bit-exact from the integer k
std::vector<double> host_dt(const uint32_t *edt_k, size_t N, double res) {
    std::vector<double> dt(N);
    for (size_t i = 0; i < N; ++i) dt[i] = res * std::sqrt((double)edt_k[i]);
    return dt;
}

}  // namespace f110

// Test hook: the padded (kind 1) or row-major (kind 0) table f110_create
// would upload for this EDT, on the host.  Returns the table's length in
// doubles (0 when it is not built: the padded table's limits), fills out when
// out_len is enough, and meta = {rows, cols, zero-cell byte offset}.
extern "C" int64_t f110_host_map_table(const uint32_t *edt_k, int32_t H, int32_t W, double res, int32_t kind,
                                       int32_t pad, double *out, int64_t out_len, int64_t meta[3]) {
    if (!edt_k || H <= 0 || W <= 0 || !(res > 0)) return fail(F110_E_INVALID, "f110_host_map_table: bad arguments");
    const std::vector<double> d = host_dt(edt_k, (size_t)H * W, res);
    size_t Wp = 0, Hp = 0;
    const std::vector<double> t = kind == 1 ? host_padded_table(H, W, pad, d, Wp, Hp) : host_rowmajor_table(H, W, d, Wp, Hp);
    if (meta) {
        meta[0] = (int64_t)Hp;
        meta[1] = (int64_t)Wp;
        meta[2] = t.empty() ? -1 : (int64_t)(Wp * Hp * 8);
    }
    if (out && out_len >= (int64_t)t.size()) std::copy(t.begin(), t.end(), out);
    return (int64_t)t.size();
}

extern "C" int f110_host_cell_index(int32_t H, int32_t W, double resolution, const double origin[3],
                                    const double *xy, int64_t n, int64_t *lin_out) {
    if (H <= 0 || W <= 0 || !(resolution > 0) || !origin || (n > 0 && (!xy || !lin_out)))
        return fail(F110_E_INVALID, "f110_host_cell_index: bad arguments");
    const MapView m = make_map_view(nullptr, H, W, resolution, origin);
    const TiledMapView t = make_tiled_view(m, nullptr);
    const bool rot = !(t.os == 0.0 && t.oc == 1.0);
    for (int64_t i = 0; i < n; ++i) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        lin_out[3 * i] = cell_index(m, x, y);
        lin_out[3 * i + 1] = cell_index_fast(m, x, y);
        const int32_t q = rot ? tiled_cell<true>(t, x, y) : tiled_cell<false>(t, x, y);
        const int32_t tile = q >> 4, within = q & 15;  // column-major within the tile (tiled_index)
        const int64_t r = (int64_t)(tile / t.wt) * 4 + (within & 3);
        const int64_t c = (int64_t)(tile % t.wt) * 4 + (within >> 2);
        lin_out[3 * i + 2] = r * W + c;
    }
    return F110_OK;
}

// ------------------------------------------------------ the ray launch ------
namespace f110 {

// k_rays_fxs's waves per car for `cars` traced at once on the device (one context's cars, or the
// device's under f110_set_device_share).  Round 5 (profiles/r05_ab/shard_rules_*.jsonl, env-steps/s,
// 1 / 2 / 3 waves per car; k_rays_fx in brackets): one context 65536 90.5 / 87.6 / 82.9 M, 32768
// 77.4 / 77.2 / 73.9, 16384 60.9 / 63.1 / 62.0, 8192 46.7 / 49.0 / 49.6 (40.2), 4096 31.8 / 34.9 /
// 35.9 (29.6); 4 sub-shards 16384 73.7 / 74.4 / 74.0, 8192 57.1 / 60.5 / 63.0 (52.0), 4096 36.9 /
// 41.1 / 42.2 (36.1); two-agent envs alike (8192 x 2: 25.4 / 26.3 / 25.8).  A car split over more
// waves shortens the longest car's chain, the launch's tail where the grid is one round deep; where
// it is many rounds deep the extra waves re-fetch the car's neighbourhood on other CUs.
static int32_t refill_waves(int64_t cars) { return cars >= 32768 ? 1 : cars >= 16384 ? 2 : 3; }

// The size rules, the one place that has them: the knobs of a context of `own` cars on a
// device that traces device_cars at once in `contexts` contexts.  f110_create applies them with
// device_cars = own and one context, f110_set_device_share with the caller's figures.
RayRules ray_rules(int64_t own, int64_t device_cars, int32_t contexts, int32_t kernel, bool pad_allowed) {
    RayRules r{1, 0, 0, 0};
    if (kernel != 3) {
        // one ray per lane, no refill.  Heavy-first (the tiled kernels) pays where one ray grid is a few
        // rounds of waves deep (16384 cars: 0.281 vs 0.287 ms), costs where it is deep (65536: 1.288 vs
        // 1.251 ms) or one round or less (8192 cars 0.172 vs 0.167, 4096 cars 0.124 vs 0.109 ms;
        // profiles/r02_ray_ab/ab_heavy.json, profiles/r03_ab/small_shards.json), and beside other
        // contexts, which fill this one's tail
        r.heavy_first = contexts == 1 && own > 8192 && own < 32768;
        return r;
    }
    // k_rays_fxs (one or a few waves per car, two chunk slots with refill, padded EDT) at every size
    // since round 5, when closed slots stopped gathering; it takes no heavy-first list
    // and needs 2 rays per lane.  Without the padded table (F110_FX_PAD=0) the old size rule: 2 rays
    // per lane from 12288 cars
    r.lanes = pad_allowed || device_cars >= 12288 ? 2 : 1;
    r.refill = pad_allowed ? refill_waves(device_cars) : 0;
    // the LDS theta table's 8-wave blocks leave idle slots that other contexts fill: it pays beside
    // them (65536 cars in 2 sub-shards 89.5 -> 95.9 M) but not alone (one context 88.3 -> 87.2 M,
    // DESIGN §3.14)
    r.fxs_lds = contexts > 1;
    return r;
}

// The ray launch of a context, the one place that decides it:
//   kernel 1:  k_rays_tiled in flat ray order, kRayBlock rays per block;
//   kernel 2:  k_rays_tiled chunked: HB heavy-first blocks (steps of a context that keeps a list),
//              then a block per (chunk, wpb cars); also kernel 3 on a rotated map;
//   kernel 3:  the fixed-point kernels (f110_create checked their preconditions: axis-aligned map,
//              one-wave blocks, W, H < 2^21, |origin / res| < 2^20, EDT entries 0 or > eps):
//              k_rays_fx (1 ray per lane, clamped table), k_rays_fxn<2> (2 rays per lane, a block
//              per chunk group, on the padded table where it exists) or, for unmasked launches
//              of a context with refill waves, fxs_ok and no heavy-first, k_rays_fxs.
RayPlan plan_ray_launch(const RayKnobs &k, bool masked) {
    const int EA = k.E * k.A, chunks = (k.B + 63) / 64;
    const bool single = k.A == 1, fx = k.kernel == 3 && !k.rotated && k.ray_wpb == 1 && k.has_rm;
    const bool pair = fx && k.lanes == 2, pad = pair && k.has_rmp;  // k_rays_fxn<2>; on the padded table
    RayPlan p{};
    p.rot = k.rotated != 0;
    p.mask = masked;
    p.handoff = !single;  // HANDOFF for A >= 2
    p.family = F110_RAY_TILED_FLAT;
    p.table = pad ? F110_TABLE_PADDED : fx ? F110_TABLE_ROWMAJOR : F110_TABLE_TILED;
    p.grid = (uint32_t)(((int64_t)EA * k.B + kRayBlock - 1) / kRayBlock);
    p.block = (uint32_t)kRayBlock;
    if (k.kernel < 2) return p;
    p.family = pad ? F110_RAY_FXN_PADDED : pair ? F110_RAY_FXN_CLAMPED : fx ? F110_RAY_FX : F110_RAY_TILED_CHUNKED;
    p.wpb = k.ray_wpb;
    p.G4 = (EA + p.wpb - 1) / p.wpb;
    p.nch = pair ? (chunks + 1) / 2 : chunks;  // k_rays_fxn: chunk groups per car (heavy list / wcost units)
    p.wcost = k.heavy_list && k.heavy_on;  // the cost bytes feed the next step's heavy-first list only
    if (k.heavy_use && !masked) p.HB = (k.heavy_cap + p.wpb - 1) / p.wpb;
    p.trace = k.wtrace && !fx && !k.rotated && !masked;  // f110_debug_wave_trace
    p.grid = (uint32_t)(p.HB + p.G4 * p.nch);
    p.block = 64u * (uint32_t)p.wpb;
    if (pad && k.refill > 0 && k.fxs_ok && !masked && p.HB == 0 && !p.wcost) {
        // k_rays_fxs: one or a few waves per car, two chunk slots with refill (no heavy-first)
        p.family = F110_RAY_FXS;
        p.lds = single && k.fxs_lds && k.theta_dis <= kFxsLdsTheta;
        p.count = k.count_slots != 0;  // f110_debug_set_simt: the variant that counts lookups, rays, lane slots
        p.G4 = std::min(k.refill, chunks);  // waves per car
        p.geo_ready = !single && k.has_geo;  // leading geometry items (a multiple of 8: XCD mapping kept)
        p.geo_blocks = p.geo_ready ? ((EA * (k.A - 1) + 63) / 64 + 7) / 8 * 8 : 0;
        const int wpb = p.lds ? kFxsWaves : 1;  // k_rays_fxs's work items per block
        p.grid = (uint32_t)((p.geo_blocks + EA * p.G4 + wpb - 1) / wpb);
        p.block = 64u * (uint32_t)wpb;
    }
    return p;
}

}  // namespace f110

extern "C" int f110_host_ray_rules(int64_t own_cars, int64_t device_cars, int32_t contexts, int32_t kernel,
                                   int32_t pad_allowed, int32_t out[4]) {
    if (!out || contexts < 1 || own_cars < 1 || device_cars < own_cars || kernel < 1 || kernel > 3)
        return fail(F110_E_INVALID, "f110_host_ray_rules: bad arguments");
    const RayRules r = ray_rules(own_cars, device_cars, contexts, kernel, pad_allowed != 0);
    std::memcpy(out, &r, sizeof r);  // {lanes, refill, heavy_first, fxs_lds}
    return F110_OK;
}

extern "C" int f110_host_ray_plan(const f110_ray_knobs *in, int32_t masked, f110_ray_plan *out) {
    if (!in || !out || in->E < 1 || in->A < 1 || in->B < 2 || in->ray_wpb < 1)
        return fail(F110_E_INVALID, "f110_host_ray_plan: bad arguments");
    *out = plan_ray_launch(*in, masked != 0);
    return F110_OK;
}

// ------------------------------------------------- per-env vehicle params --
namespace f110 {

const char *const kParamNames[19] = {"mu", "C_Sf", "C_Sr", "lf", "lr", "h", "m", "I", "s_min", "s_max",
                                     "sv_min", "sv_max", "v_switch", "a_max", "v_min", "v_max",
                                     "width", "length", "lidar_max"};

int check_param_ranges(const char *who, const f110_params *lo, const f110_params *hi, const f110_params *agents,
                       int32_t n_agents) {
    if (!lo || !hi || !agents || n_agents <= 0) return fail(F110_E_INVALID, std::string(who) + ": null argument");
    for (int i = 0; i < n_agents; ++i) {
        const std::string where = " (agent " + std::to_string(i) + ")";
        int rc = check_param_row(who, lo[i], agents[i], [&] { return " lo" + where; });
        if (rc == F110_OK) rc = check_param_row(who, hi[i], agents[i], [&] { return " hi" + where; });
        if (rc != F110_OK) return rc;
        for (int k = 0; k < kDynFields; ++k) {
            if (fields(lo[i])[k] > fields(hi[i])[k])
                return fail(F110_E_INVALID, std::string(who) + ": " + kParamNames[k] + where + " has lo > hi");
            if (!std::isfinite(fields(hi[i])[k] - fields(lo[i])[k]))
                return fail(F110_E_INVALID, std::string(who) + ": " + kParamNames[k] + where + " hi - lo is not finite");
        }
    }
    return F110_OK;
}

}  // namespace f110

extern "C" int f110_host_check_param_ranges(const f110_params *lo, const f110_params *hi, const f110_params *agent_params,
                                            int32_t n_agents) {
    return check_param_ranges("f110_host_check_param_ranges", lo, hi, agent_params, n_agents);
}

extern "C" int f110_host_param_draw(uint64_t seed, int64_t env, int32_t agent, uint64_t episode, const f110_params *lo,
                                    const f110_params *hi, f110_params *out) {
    if (!lo || !hi || !out || agent < 0 || agent >= kMaxAgents)
        return fail(F110_E_INVALID, "f110_host_param_draw: null argument or bad agent");
    double range[2 * kDynFields], v[kDynFields];
    std::memcpy(range, lo, sizeof(double) * kDynFields);
    std::memcpy(range + kDynFields, hi, sizeof(double) * kDynFields);
    param_draw(seed, (uint64_t)env, agent, episode, range, v);
    *out = *lo;
    std::memcpy(out, v, sizeof(v));
    return F110_OK;
}

// ---------------------------------------------------- spawn randomization --
namespace f110 {

int check_spawn_ranges(const char *who, const f110_spawn_range *ranges, int32_t n_agents, int32_t n_spawn) {
    if (!ranges || n_agents <= 0) return fail(F110_E_INVALID, std::string(who) + ": null argument");
    for (int i = 0; i < n_agents; ++i) {
        const f110_spawn_range &r = ranges[i];
        const std::string where = " (agent " + std::to_string(i) + ")";
        const auto bad = [&](const char *field, const char *what) {
            return fail(F110_E_INVALID, std::string(who) + ": " + field + where + " " + what);
        };
        const struct {
            const char *name;
            const double *v;
        } pairs[3] = {{"lateral", r.lateral}, {"heading", r.heading}, {"speed", r.speed}};
        for (const auto &p : pairs) {
            if (!std::isfinite(p.v[0]) || !std::isfinite(p.v[1])) return bad(p.name, "is not finite");
            if (p.v[0] > p.v[1]) return bad(p.name, "has lo > hi");
            if (!std::isfinite(p.v[1] - p.v[0])) return bad(p.name, "hi - lo is not finite");
        }
        if (r.gap[0] < 0 || r.gap[1] < 0) return bad("gap", "is negative");
        if (r.gap[0] > r.gap[1]) return bad("gap", "has lo > hi");
        if (!std::isfinite(r.behind)) return bad("behind", "is not finite");
        if (r.behind < 0.0 || r.behind > 1.0) return bad("behind", "is outside [0, 1]");
        if (!std::isfinite(r.clearance)) return bad("clearance", "is not finite");
        if (r.clearance < 0.0) return bad("clearance", "is negative");
        if (r.gap[1] > 0 && n_spawn <= 0) return bad("gap", "is non-zero on a context without a spawn table");
    }
    return F110_OK;
}

}  // namespace f110

extern "C" int f110_host_check_spawn_ranges(const f110_spawn_range *ranges, int32_t n_agents, int32_t n_spawn) {
    return check_spawn_ranges("f110_host_check_spawn_ranges", ranges, n_agents, n_spawn);
}

extern "C" int f110_host_spawn_rows(const f110_spawn_range *ranges, int32_t n_agents, uint64_t seed, uint64_t ctx_seed,
                                    const double *edt, int32_t H, int32_t W, double resolution, const double origin[3],
                                    const double *spawn, int32_t n_spawn, const double *poses, const int32_t *rows,
                                    const int64_t *envs, const uint64_t *episodes, int64_t n, int32_t reset_f32,
                                    double *out, int32_t *rows_out) {
    const char *who = "f110_host_spawn_rows";
    if (!edt || H <= 0 || W <= 0 || !(resolution > 0) || !origin || n < 0 || (n > 0 && (!envs || !out)))
        return fail(F110_E_INVALID, std::string(who) + ": bad arguments");
    if (!poses && (!spawn || n_spawn <= 0))
        return fail(F110_E_INVALID, std::string(who) + ": an autoreset needs a spawn table");
    const int rc = check_spawn_ranges(who, ranges, n_agents, spawn ? n_spawn : 0);
    if (rc != F110_OK) return rc;
    if (!poses)
        for (int64_t i = 0; i < n; ++i) {
            if (rows && (rows[i] < 0 || rows[i] >= n_spawn)) return fail(F110_E_INVALID, std::string(who) + ": row out of range");
            if (!rows && (!episodes || episodes[i] == 0))
                return fail(F110_E_INVALID, std::string(who) + ": an autoreset's episode is >= 1");
        }
    const MapView m = make_map_view(edt, H, W, resolution, origin);
    const size_t A = (size_t)n_agents;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t env = (uint64_t)envs[i], episode = episodes ? episodes[i] : 0;
        for (int ag = 0; ag < n_agents; ++ag) {
            const f110_spawn_range &r = ranges[ag];
            const SpawnDraws w = spawn_draws(seed, env, ag, episode, r);
            const double *pz;
            int32_t row = -1;
            if (poses) {
                pz = poses + ((size_t)i * A + (size_t)ag) * 3;
            } else {
                uint32_t k = rows ? (uint32_t)rows[i] : spawn_draw(ctx_seed, env, episode - 1) % (uint32_t)n_spawn;
                int col = ag;
                if (!spawn_own_column(r)) {
                    k = spawn_shift_row(k, w.mag, w.behind, (uint32_t)n_spawn);
                    col = 0;
                }
                row = (int32_t)k;
                pz = spawn + ((size_t)k * A + (size_t)col) * 3;
            }
            spawn_pose(m, pz[0], pz[1], pz[2], w, r.clearance, reset_f32 != 0, out + ((size_t)i * A + (size_t)ag) * 4);
            if (rows_out) rows_out[(size_t)i * A + (size_t)ag] = row;
        }
    }
    return F110_OK;
}

// ------------------------------------------- episode limits and statistics --
namespace f110 {

int check_episode_limits(const char *who, int64_t max_steps, double stall_speed, int32_t stall_steps) {
    if (max_steps < 0) return fail(F110_E_INVALID, std::string(who) + ": max_steps is negative");
    if (stall_steps < 0) return fail(F110_E_INVALID, std::string(who) + ": stall_steps is negative");
    if (!std::isfinite(stall_speed)) return fail(F110_E_INVALID, std::string(who) + ": stall_speed is not finite");
    if (stall_speed < 0) return fail(F110_E_INVALID, std::string(who) + ": stall_speed is negative");
    return F110_OK;
}

int check_episode_args(const char *who, const double *rewards, const uint8_t *terminated, const uint8_t *was_reset,
                       int64_t n_envs, const f110_episode_state *state, const f110_episode_totals *totals) {
    if (!rewards || !terminated || !was_reset || !state || !totals)
        return fail(F110_E_INVALID, std::string(who) + ": null argument");
    if (n_envs < 0 || episode_blocks(n_envs) > 0x7fffffff) return fail(F110_E_INVALID, std::string(who) + ": bad n_envs");
    return F110_OK;
}

}  // namespace f110

extern "C" int f110_host_check_episode_limits(int64_t max_steps, double stall_speed, int32_t stall_steps) {
    return check_episode_limits("f110_host_check_episode_limits", max_steps, stall_speed, stall_steps);
}

extern "C" int f110_host_episode_stats(const double *rewards, const uint8_t *terminated, const uint8_t *truncated,
                                       const uint8_t *was_reset, int64_t n_envs, f110_episode_state *state,
                                       double *last_return, int32_t *last_length, uint8_t *finished,
                                       f110_episode_totals *totals) {
    const int rc = check_episode_args("f110_host_episode_stats", rewards, terminated, was_reset, n_envs, state, totals);
    if (rc != F110_OK) return rc;
    EpisodePart call = {0, 0, 0, 0, 0.0, 0.0, 0.0};
    for (int64_t e = 0; e < n_envs; ++e) {
        const int code = episode_update(rewards[e], terminated[e], truncated ? truncated[e] : 0, was_reset[e], state[e]);
        if (finished) finished[e] = code ? 1 : 0;
        if (code) {
            if (last_return) last_return[e] = state[e].ret;
            if (last_length) last_length[e] = state[e].len;
        }
        episode_merge(call, episode_part(code, state[e]));
    }
    episode_totals_add(*totals, call);
    return F110_OK;
}

// ---- f110_track's arrays (rewards.py / track_progress.py) --------------------
namespace f110 {

// track_progress.py:29-46: seg = diff(xy); seg_len = norm(seg, axis=1) =
// sqrt(dx*dx + dy*dy); s = [0, cumsum(seg_len)]; tan = seg / max(seg_len,
// 1e-12); nrm = (-tan_y, tan_x); mid = (xy[:-1] + xy[1:]) * 0.5
void track_arrays(const double *xy, int32_t n, std::vector<double> &s, std::vector<double> &tan,
                  std::vector<double> &nrm, std::vector<double> &mid) {
    s.assign((size_t)n, 0.0);
    tan.assign((size_t)2 * (n - 1), 0.0);
    nrm.assign((size_t)2 * (n - 1), 0.0);
    mid.assign((size_t)2 * (n - 1), 0.0);
    double acc = 0.0;
    for (int32_t i = 0; i + 1 < n; ++i) {
        const double dx = xy[2 * i + 2] - xy[2 * i], dy = xy[2 * i + 3] - xy[2 * i + 1];
        const double len = std::sqrt(dx * dx + dy * dy);
        acc = acc + len;
        s[(size_t)i + 1] = acc;
        const double den = len > 1e-12 ? len : 1e-12;
        tan[2 * (size_t)i] = dx / den;
        tan[2 * (size_t)i + 1] = dy / den;
        nrm[2 * (size_t)i] = -tan[2 * (size_t)i + 1];
        nrm[2 * (size_t)i + 1] = tan[2 * (size_t)i];
        mid[2 * (size_t)i] = (xy[2 * i] + xy[2 * i + 2]) * 0.5;
        mid[2 * (size_t)i + 1] = (xy[2 * i + 1] + xy[2 * i + 3]) * 0.5;
    }
}

// uniform grid over the segment midpoints (reward kernel's kd.query):
// cells of 16 median segment lengths (a 3x3 block then holds ~50
// midpoints of a centerline through it; the kernel widens the block when
// the 5th nearest is not provably inside), one cell of margin on every side
TrackGrid track_grid(const double *xy, int32_t n, const std::vector<double> &mid) {
    TrackGrid g;
    if (n < 2) return g;
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int32_t i = 0; i + 1 < n; ++i) {
        mnx = std::min(mnx, mid[2 * (size_t)i]);
        mxx = std::max(mxx, mid[2 * (size_t)i]);
        mny = std::min(mny, mid[2 * (size_t)i + 1]);
        mxy = std::max(mxy, mid[2 * (size_t)i + 1]);
    }
    std::vector<double> seg;
    for (int32_t i = 0; i + 1 < n; ++i)
        seg.push_back(std::hypot(xy[2 * (size_t)i + 2] - xy[2 * (size_t)i], xy[2 * (size_t)i + 3] - xy[2 * (size_t)i + 1]));
    std::nth_element(seg.begin(), seg.begin() + seg.size() / 2, seg.end());
    const double med = seg[seg.size() / 2];
    const double ext = std::max(mxx - mnx, mxy - mny);
    // at most 4096 cells a side; a degenerate spacing falls back to ext / 64
    const double h = std::max(std::isfinite(med) && med > 0.0 ? 16.0 * med : ext / 64.0, ext / 4000.0);
    if (h > 0.0 && std::isfinite(h) && std::isfinite(mnx) && std::isfinite(mny) && std::isfinite(mxx) && std::isfinite(mxy) &&
        (mxx - mnx) / h < 4096 && (mxy - mny) / h < 4096) {
        g.gh = h;
        g.gx0 = mnx - h;
        g.gy0 = mny - h;
        g.gnx = (int32_t)((mxx - g.gx0) / h) + 2;
        g.gny = (int32_t)((mxy - g.gy0) / h) + 2;
        const size_t nc = (size_t)g.gnx * g.gny;
        std::vector<int32_t> cell((size_t)n - 1);
        g.cstart.assign(nc + 1, 0);
        for (int32_t i = 0; i + 1 < n; ++i) {
            const int32_t ci = (int32_t)((mid[2 * (size_t)i] - g.gx0) / h);
            const int32_t cj = (int32_t)((mid[2 * (size_t)i + 1] - g.gy0) / h);
            cell[(size_t)i] = cj * g.gnx + ci;
            ++g.cstart[(size_t)cell[(size_t)i] + 1];
        }
        for (size_t c = 0; c < nc; ++c) g.cstart[c + 1] += g.cstart[c];
        g.citems.assign((size_t)n - 1, 0);
        std::vector<int32_t> fill(g.cstart.begin(), g.cstart.end() - 1);
        for (int32_t i = 0; i + 1 < n; ++i) g.citems[(size_t)fill[(size_t)cell[(size_t)i]]++] = i;
        g.cmid.resize(2 * g.citems.size());
        for (size_t q = 0; q < g.citems.size(); ++q) {
            g.cmid[2 * q] = mid[2 * (size_t)g.citems[q]];
            g.cmid[2 * q + 1] = mid[2 * (size_t)g.citems[q] + 1];
        }
    }
    return g;
}

// ---- n-step returns ---------------------------------------------------------
int check_nstep_args(const char *fn, int64_t n_envs, int32_t n_step, double gamma, int32_t obs_dim, int32_t act_dim) {
    if (n_step < 1 || n_step > kNstepMax) return fail(F110_E_INVALID, std::string(fn) + ": n_step must be in [1, 16]");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0)
        return fail(F110_E_INVALID, std::string(fn) + ": gamma must be finite and in [0, 1]");
    if (n_envs <= 0 || n_envs * n_step >= (int64_t)1 << 31)
        return fail(F110_E_INVALID, std::string(fn) + ": n_envs must be positive (n_envs * n_step < 2^31)");
    if (obs_dim <= 0 || act_dim <= 0 || act_dim > 256)
        return fail(F110_E_INVALID, std::string(fn) + ": obs_dim > 0 and 0 < act_dim <= 256");
    return F110_OK;
}

int check_nstep_capacity(const char *fn, int64_t n_envs, int32_t n_step, int64_t capacity) {
    if (n_envs * n_step > capacity)
        return fail(F110_E_INVALID, std::string(fn) + ": n_envs * n_step must not exceed the replay's capacity");
    return F110_OK;
}

void nstep_powers(double gamma, int n, double *pw) {  // sequential products
    pw[0] = 1.0;
    for (int i = 1; i <= n; ++i) pw[i] = pw[i - 1] * gamma;
}

// ---- action repeat ------------------------------------------------------------
int check_repeat_args(const char *fn, int64_t n_envs, int32_t repeat, double gamma, int32_t obs_dim, int32_t act_dim) {
    if (repeat < 1 || repeat > kRepeatMax) return fail(F110_E_INVALID, std::string(fn) + ": repeat must be in [1, 64]");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0)
        return fail(F110_E_INVALID, std::string(fn) + ": gamma must be finite and in [0, 1]");
    if (n_envs <= 0 || n_envs >= (int64_t)1 << 31)
        return fail(F110_E_INVALID, std::string(fn) + ": n_envs must be positive (and below 2^31)");
    if (obs_dim <= 0 || act_dim <= 0 || act_dim > 256)
        return fail(F110_E_INVALID, std::string(fn) + ": obs_dim > 0 and 0 < act_dim <= 256");
    return F110_OK;
}

int check_repeat_capacity(const char *fn, int64_t n_envs, int64_t capacity) {
    if (n_envs > capacity)
        return fail(F110_E_INVALID, std::string(fn) + ": n_envs must not exceed the replay's capacity");
    return F110_OK;
}

}  // namespace f110

extern "C" int f110_host_repeat_hold(int64_t n_envs, int32_t obs_dim, int32_t act_dim, const int32_t *k, float *s_obs,
                                     float *s_act, const float *obs, float *act, uint8_t *decision) {
    if (n_envs <= 0 || obs_dim <= 0 || act_dim <= 0 || act_dim > 256)
        return fail(F110_E_INVALID, "f110_host_repeat_hold: n_envs > 0, obs_dim > 0 and 0 < act_dim <= 256");
    if (!k || !s_obs || !s_act || !obs || !act) return fail(F110_E_INVALID, "f110_host_repeat_hold: null argument");
    const size_t D = (size_t)obs_dim, A = (size_t)act_dim;
    for (int64_t e = 0; e < n_envs; ++e) {
        if (k[e] == 0) {
            std::copy(obs + e * D, obs + (e + 1) * D, s_obs + e * D);
            std::copy(act + e * A, act + (e + 1) * A, s_act + e * A);
        } else {
            std::copy(s_act + e * A, s_act + (e + 1) * A, act + e * A);
        }
        if (decision) decision[e] = k[e] == 0 ? 1 : 0;
    }
    return F110_OK;
}

extern "C" int f110_host_repeat_push(int64_t n_envs, int32_t repeat, double gamma, int32_t obs_dim, int32_t act_dim,
                                     int64_t capacity, int32_t *k, double *ret, const float *s_obs, const float *s_act,
                                     const double *reward, const float *next_obs, const uint8_t *terminated,
                                     const uint8_t *truncated, const uint8_t *was_reset, float *out_obs, float *out_act,
                                     float *out_reward, float *out_next_obs, float *out_done, int64_t *out_count) {
    int rc = check_repeat_args("f110_host_repeat_push", n_envs, repeat, gamma, obs_dim, act_dim);
    if (rc == F110_OK && capacity > 0) rc = check_repeat_capacity("f110_host_repeat_push", n_envs, capacity);
    if (rc != F110_OK) return rc;
    if (!k || !ret || !s_obs || !s_act || !reward || !next_obs || !terminated || !was_reset || !out_obs || !out_act ||
        !out_reward || !out_next_obs || !out_done || !out_count)
        return fail(F110_E_INVALID, "f110_host_repeat_push: null argument");
    const size_t D = (size_t)obs_dim, A = (size_t)act_dim;
    double pw[kRepeatMax + 1];
    nstep_powers(gamma, repeat, pw);
    int64_t row = 0;
    for (int64_t e = 0; e < n_envs; ++e) {
        float e_reward = 0.0f, e_done = 0.0f;
        if (!repeat_update(repeat, pw, reward[e], terminated[e], truncated ? truncated[e] : 0, was_reset[e], k[e], ret[e],
                           e_reward, e_done))
            continue;
        std::copy(s_obs + e * D, s_obs + (e + 1) * D, out_obs + row * D);
        std::copy(s_act + e * A, s_act + (e + 1) * A, out_act + row * A);
        std::copy(next_obs + e * D, next_obs + (e + 1) * D, out_next_obs + row * D);
        out_reward[row] = e_reward;
        out_done[row] = e_done;
        ++row;
    }
    *out_count = row;
    return F110_OK;
}

extern "C" int f110_host_nstep(int64_t n_envs, int32_t n_step, double gamma, int32_t obs_dim, int32_t act_dim,
                               int64_t capacity, int32_t *len, int32_t *head, double *ret, int32_t *k, float *win_obs,
                               float *win_act, const float *obs, const float *act, const double *reward,
                               const float *next_obs, const uint8_t *terminated, const uint8_t *truncated,
                               const uint8_t *was_reset, float *out_obs, float *out_act, float *out_reward,
                               float *out_next_obs, float *out_done, int64_t *out_count) {
    int rc = check_nstep_args("f110_host_nstep", n_envs, n_step, gamma, obs_dim, act_dim);
    if (rc == F110_OK && capacity > 0) rc = check_nstep_capacity("f110_host_nstep", n_envs, n_step, capacity);
    if (rc != F110_OK) return rc;
    if (!len || !head || !ret || !k || !win_obs || !win_act || !obs || !act || !reward || !next_obs || !terminated ||
        !was_reset || !out_obs || !out_act || !out_reward || !out_next_obs || !out_done || !out_count)
        return fail(F110_E_INVALID, "f110_host_nstep: null argument");
    const int n = n_step;
    const size_t D = (size_t)obs_dim, A = (size_t)act_dim;
    double pw[kNstepMax + 1];
    nstep_powers(gamma, n, pw);
    int64_t row = 0;
    for (int64_t e = 0; e < n_envs; ++e) {
        int32_t e_slot[kNstepMax], store;
        float e_reward[kNstepMax], e_done[kNstepMax];
        const int cnt = nstep_update(n, pw, reward[e], terminated[e], truncated ? truncated[e] : 0, was_reset[e], len[e],
                                     head[e], ret + e * n, k + e * n, e_slot, e_reward, e_done, store);
        for (int j = 0; j < cnt; ++j, ++row) {
            const float *so = e_slot[j] < 0 ? obs + e * D : win_obs + ((size_t)e * n + e_slot[j]) * D;
            const float *sa = e_slot[j] < 0 ? act + e * A : win_act + ((size_t)e * n + e_slot[j]) * A;
            std::copy(so, so + D, out_obs + row * D);
            std::copy(sa, sa + A, out_act + row * A);
            std::copy(next_obs + e * D, next_obs + (e + 1) * D, out_next_obs + row * D);
            out_reward[row] = e_reward[j];
            out_done[row] = e_done[j];
        }
        if (store >= 0) {
            std::copy(obs + e * D, obs + (e + 1) * D, win_obs + ((size_t)e * n + store) * D);
            std::copy(act + e * A, act + (e + 1) * A, win_act + ((size_t)e * n + store) * A);
        }
    }
    *out_count = row;
    return F110_OK;
}

// ---- self-play: the flat observation from an agent's seat ---------------------
extern "C" int f110_host_agent_obs(const float *scans, int64_t scan_env_stride, const float *obs, int64_t obs_stride,
                                   int64_t n_envs, int32_t n_agents, int32_t n_beams, int32_t agent, float lidar_max,
                                   float *out, int64_t out_stride) {
    if (agent_obs_bad_args(scans, scan_env_stride, obs, obs_stride, n_envs, n_agents, n_beams, agent, out, out_stride))
        return fail(F110_E_INVALID, "f110_host_agent_obs: bad arguments");
    const int64_t B = n_beams;
    for (int64_t e = 0; e < n_envs; ++e) {
        const float *s = scans + e * scan_env_stride + agent * B;
        const float *p = obs + e * obs_stride + B;
        float *o = out + e * out_stride;
        for (int64_t b = 0; b < B; ++b) o[b] = obs_scan_value(s[b], lidar_max);
        for (int g = 0; g < n_agents; ++g) {  // the seat's own pose group first, then the others ascending
            const int src = g == 0 ? agent : (g <= agent ? g - 1 : g);
            std::copy(p + 4 * src, p + 4 * src + 4, o + B + 4 * g);
        }
    }
    return F110_OK;
}

// ---- scan observation (f110_scan_obs.hip; the row rule: f110_scan_obs.h) ----------------------
extern "C" void f110_default_scan_obs_params(f110_scan_obs_params *p) {
    if (!p) return;
    *p = f110_scan_obs_params{};
    p->n_bins = 108;
    p->n_frames = 1;
    p->stride = 1;
    p->reduce = 0;
    p->keep_mid = 1;
}

extern "C" int32_t f110_scan_obs_width(const f110_scan_obs_params *params, int32_t n_beams, int32_t n_mid,
                                       int32_t n_tail) {
    if (scan_obs_bad_shape(params, n_beams, n_mid, n_tail)) return -1;
    return scan_obs_width(*params, n_mid, n_tail);
}

extern "C" int f110_host_scan_obs_push(const f110_scan_obs_params *params, int64_t n_envs, int32_t n_beams,
                                       int32_t n_mid, int32_t n_tail, const float *rows, int64_t row_stride,
                                       const uint8_t *reset, float *ring, int32_t *head, float *out,
                                       int64_t out_stride) {
    const char *bad = scan_obs_bad_shape(params, n_beams, n_mid, n_tail);
    if (!bad && n_envs < 1) bad = "n_envs must be at least 1";
    if (!bad && (!ring || !head)) bad = "null ring or head";
    const f110_scan_obs_params &P = *params;
    if (!bad) bad = scan_obs_bad_push(n_envs, n_beams + n_mid + n_tail, scan_obs_width(P, n_mid, n_tail), rows,
                                      row_stride, out, out_stride);
    if (bad) return fail(F110_E_INVALID, std::string("f110_host_scan_obs_push: ") + bad);
    const int32_t B = n_beams, K = P.n_bins, F = P.n_frames, S = P.stride, D = scan_obs_depth(P);
    for (int64_t e = 0; e < n_envs; ++e)
        if (head[e] < -1 || head[e] >= D)
            return fail(F110_E_INVALID, "f110_host_scan_obs_push: a head outside [-1, D)");
    const int32_t n_copy = (P.keep_mid ? n_mid : 0) + n_tail;
    for (int64_t e = 0; e < n_envs; ++e) {
        const float *row = rows + e * row_stride;
        float *o = out + e * out_stride;
        float *rg = ring + (size_t)e * D * K;
        bool refill;
        const int32_t h = scan_obs_advance(head[e], reset ? reset[e] : 0, D, refill);
        for (int32_t k = 0; k < K; ++k) {
            const float v = scan_obs_pool(row, scan_obs_edge(k, B, K), scan_obs_edge(k + 1, B, K), P.reduce);
            if (refill) {
                for (int32_t d = 0; d < D; ++d) rg[(size_t)d * K + k] = v;
            } else {
                rg[(size_t)h * K + k] = v;
            }
        }
        head[e] = h;
        for (int32_t j = 0; j < F; ++j) {
            const float *slot = rg + (size_t)scan_obs_slot(h, j, S, D) * K;
            std::copy(slot, slot + K, o + (size_t)j * K);
        }
        const float *src = row + B + (P.keep_mid ? 0 : n_mid);
        std::copy(src, src + n_copy, o + (size_t)F * K);
    }
    return F110_OK;
}

// ---- sensor randomization (f110_sensor.hip; the row rule: f110_sensor.h) ----------------------
extern "C" void f110_default_sensor_params(f110_sensor_params *p) {
    if (!p) return;
    *p = f110_sensor_params{};  // every sigma, dropout, blackout and quant (0, 0)
    p->scale[0] = p->scale[1] = 1.0f;
}

extern "C" int f110_host_check_sensor_params(const f110_sensor_params *params, int32_t n_beams) {
    const char *bad = n_beams < 1 || n_beams > kSensorMaxBeams ? "n_beams must be in [1, 4096]"
                                                               : sensor_bad_params(params, n_beams);
    if (bad) return fail(F110_E_INVALID, std::string("f110_host_check_sensor_params: ") + bad);
    return F110_OK;
}

extern "C" int f110_host_sensor_apply(const f110_sensor_params *params, int64_t n_envs, int32_t n_beams,
                                      int32_t n_mid, int32_t n_tail, float range_max, uint64_t seed,
                                      int64_t env_offset, const uint8_t *env_mask, const float *rows,
                                      int64_t row_stride, const uint8_t *reset, float *param_rows, int32_t *episode,
                                      int32_t *step, float *out, int64_t out_stride) {
    const char *bad = sensor_bad_shape(params, n_envs, n_beams, n_mid, n_tail, range_max, env_offset);
    if (!bad && (!param_rows || !episode || !step)) bad = "null param_rows, episode or step";
    if (!bad) bad = sensor_bad_apply(n_envs, n_beams + n_mid + n_tail, rows, row_stride, out, out_stride);
    if (bad) return fail(F110_E_INVALID, std::string("f110_host_sensor_apply: ") + bad);
    for (int64_t e = 0; e < n_envs; ++e)
        if (episode[e] < -1) return fail(F110_E_INVALID, "f110_host_sensor_apply: an episode counter below -1");
    const int32_t B = n_beams, M = n_mid, W = n_beams + n_mid + n_tail;
    for (int64_t e = 0; e < n_envs; ++e) {
        const bool start = sensor_advance(episode[e], step[e], reset ? reset[e] : 0);
        const SensorKey key = sensor_key(seed, (uint64_t)(env_offset + e));
        SensorRow *held = reinterpret_cast<SensorRow *>(param_rows) + e;
        if (start) *held = sensor_draw_row(key, (uint32_t)episode[e], *params, B, range_max);
        const SensorRow r = *held;
        const float *row = rows + e * row_stride;
        float *o = out + e * out_stride;
        if (env_mask && !env_mask[e]) {
            if (o != row) std::copy(row, row + W, o);
            continue;
        }
        const uint32_t ep = (uint32_t)episode[e], st = (uint32_t)step[e];
        const bool draws = sensor_beam_draws(r);
        for (int32_t b = 0; b < B; ++b) {
            const U4 k = draws ? sensor_block(key, ep, st, (uint32_t)b) : U4{0u, 0u, 0u, 0u};
            o[b] = sensor_beam(row[b], b, r, k);
        }
        for (int32_t m = 0; m < M; ++m) {
            const U4 k = sensor_pose_draws(r, m) ? sensor_block(key, ep, st, (uint32_t)(B + m)) : U4{0u, 0u, 0u, 0u};
            o[B + m] = sensor_pose(row[B + m], m, r, k);
        }
        if (o != row) std::copy(row + B + M, row + W, o + B + M);
    }
    return F110_OK;
}
