// f110_ctx.cpp — the simulator context of libf110.so (include/f110.h): the per-device map-table
// cache, f110_create / f110_destroy, the per-step path and the context's setters and getters.
//
// Cold path (once per map): the tables of f110_host.cpp uploaded into device buffers.
// Hot path: f110_step / f110_reset fill a StepArgs and enqueue three kernels
// (k_agents, a ray kernel, a post kernel) on the caller's stream; no
// allocation, no synchronisation.  The whole of it (ray_knobs, make_step_args, ray_launch, step_n)
// lives in this translation unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_beam_runs.h"
#include "f110_ctx.h"
#include "f110_env_rows.h"
#include "f110_host.h"
#include "f110_host_util.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_step_args.h"
#include "f110_task_args.h"

using namespace f110;

static bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

static MapView map_view(const f110_ctx *c) { return make_map_view(c->dt, c->H, c->W, c->res, c->origin); }

int use_device(const f110_ctx *c) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->arena.device) HIP_TRY(hipSetDevice(c->arena.device));
    return F110_OK;
}

// ------------------------------------------------------ shared map tables --
// (MapTables, f110_ctx.h)
static std::mutex g_maps_mu;
static std::vector<MapTables *> g_maps;

static void release_map_tables(MapTables *t) {
    if (!t) return;
    std::lock_guard<std::mutex> g(g_maps_mu);
    if (--t->refs > 0) return;
    g_maps.erase(std::remove(g_maps.begin(), g_maps.end(), t), g_maps.end());
    delete t;  // (its arena frees the tables)
}

// Uploads a table (at least 16 bytes) and publishes it to *p only once the copy has succeeded (a
// failed upload frees it and leaves *p untouched): a map entry shared by other contexts never
// points at an uninitialised table.
static hipError_t upload(MapTables *t, const double **p, const std::vector<double> &h) {
    const size_t bytes = h.size() * sizeof(double);
    return t->arena.upload(p, h.data(), h.size(), bytes < 16 ? 16 - bytes : 0);
}

static hipError_t build_padded_table(MapTables *t, int32_t pad, const std::vector<double> &d) {
    size_t Wp = 0, Hp = 0;
    const std::vector<double> rmp = host_padded_table(t->H, t->W, pad, d, Wp, Hp);
    if (rmp.empty()) return hipSuccess;
    const hipError_t e = upload(t, &t->rmp, rmp);
    if (e == hipSuccess) {  // the metadata only with the table it describes
        t->rmp_w = (int32_t)Wp;
        t->rmp_h = (int32_t)Hp;
        t->rmp_P = pad;
        t->rmp_zero = (uint32_t)(Wp * Hp * 8);
    }
    return e;
}

// The tables of (device, map), built and uploaded on first use; `want_rm`
// adds the row-major table if the entry lacks it, `pad` > 0 the table padded
// by `pad` cells on every side (an entry keeps the padding it was built with:
// the kernel's per-car test reads the entry's).  Called with the device current.
static hipError_t acquire_map_tables(int device, const uint32_t *edt_k, int32_t H, int32_t W, double res,
                                     int32_t wt, int32_t tiles_h, bool want_rm, int32_t pad, MapTables **out) {
    std::lock_guard<std::mutex> g(g_maps_mu);
    const size_t N = (size_t)H * W;
    uint64_t rb;
    std::memcpy(&rb, &res, 8);
    bool share = true;
    if (const char *v = std::getenv("F110_SHARE_MAP")) share = std::atoi(v) != 0;
    MapTables *t = nullptr;
    if (share)
        for (MapTables *q : g_maps)
            if (q->shared && q->arena.device == device && q->H == H && q->W == W && q->res_bits == rb &&
                std::memcmp(q->k.data(), edt_k, N * sizeof(uint32_t)) == 0) {
                t = q;
                break;
            }
    const bool fresh = t == nullptr;
    if (fresh) {
        t = new MapTables();
        t->arena.device = device;
        t->H = H;
        t->W = W;
        t->res_bits = rb;
        t->shared = share;
        t->k.assign(edt_k, edt_k + N);
    }
    hipError_t e = hipSuccess;
    std::vector<double> dt;
    auto dt_host = [&]() -> const std::vector<double> & {
        if (dt.empty()) dt = host_dt(edt_k, N, res);
        return dt;
    };
    if (fresh) {
        e = upload(t, &t->dt, dt_host());
        if (e == hipSuccess) {
            std::vector<double> dtt((size_t)wt * tiles_h * 16, 0.0);  // padding cells are never read
            for (int r = 0; r < H; ++r)
                for (int q = 0; q < W; ++q) dtt[(size_t)tiled_index(wt, r, q)] = dt[(size_t)r * W + q];
            e = upload(t, &t->dt_tiled, dtt);
        }
    }
    if (e == hipSuccess && want_rm && !t->rm) {
        size_t Wp = 0, Hp = 0;
        e = upload(t, &t->rm, host_rowmajor_table(H, W, dt_host(), Wp, Hp));
        if (e == hipSuccess) {  // the metadata only with the table it describes
            t->rm_w = (int32_t)Wp;
            t->rm_oob = (uint32_t)(((size_t)(H - 1) * Wp + (W - 1)) * 8);
            t->rm_zero = (uint32_t)(Wp * Hp * 8);
        }
    }
    if (e == hipSuccess && pad > 0 && !t->rmp) e = build_padded_table(t, pad, dt_host());
    if (e != hipSuccess) {
        if (fresh) delete t;
        return e;
    }
    if (fresh) g_maps.push_back(t);
    ++t->refs;
    *out = t;
    return hipSuccess;
}

// the map entry's padded table (if it was built) for the context
static void adopt_padded_table(f110_ctx *c) {
    const MapTables *m = c->maps;
    if (!m || !m->rmp) return;
    c->rmp = FxTable{m->rmp, m->rmp_w, m->rmp_P, 0, m->rmp_zero};
    c->rmp_h = m->rmp_h;
}

// k_rays_fxs's offsets (kFxsBase) need q + P below 2^20 for every lookup: the padded
// table's rows and columns below 2^20 (else the refill runs k_rays_fxn instead)
static bool fxs_ok(const f110_ctx *c) { return c->rmp.dt && c->rmp.w < (1 << 20) && c->rmp_h < (1 << 20); }

// The padded EDT of k_rays_fxn / k_rays_fxs (built on first use, shared with
// the map entry): F110_FX_PAD=0 at f110_create keeps the clamped table (A/B runs).
int ensure_padded_table(f110_ctx *ctx) {
    if (!ctx->fx_pad || ctx->rmp.dt || !ctx->maps) return F110_OK;
    const double pad_q = std::ceil(ctx->cfg.max_range / ctx->res) + 8.0;
    if (pad_q > 0.0 && pad_q < 65536.0) {
        std::lock_guard<std::mutex> g(g_maps_mu);
        MapTables *t = ctx->maps;
        if (!t->rmp) {
            double res;
            std::memcpy(&res, &t->res_bits, 8);
            HIP_TRY(build_padded_table(t, (int32_t)pad_q, host_dt(t->k.data(), t->k.size(), res)));
        }
    }
    adopt_padded_table(ctx);
    return F110_OK;
}

// ------------------------------------------------------- create / destroy --
// The one way a context goes, whole (f110_destroy) or half built (a failed f110_create).
static void destroy_ctx(f110_ctx *c) {
    (void)hipSetDevice(c->arena.device);
    c->free_prof();
    c->arena.release();
    release_map_tables(c->maps);
    delete c;
}

extern "C" int f110_create(f110_ctx **out, int32_t device, const f110_config *cfg, const f110_params *params,
                           const uint32_t *edt_k, int32_t H, int32_t W, double resolution, const double origin[3],
                           const double *spawn_poses, int32_t n_spawn) {
    if (!out || !cfg || !params || !edt_k || !origin) return fail(F110_E_INVALID, "f110_create: null argument");
    *out = nullptr;
    const f110_config &C = *cfg;
    if (C.n_envs <= 0 || C.n_agents <= 0 || C.n_agents > kMaxAgents)
        return fail(F110_E_INVALID, "f110_create: n_envs must be > 0 and 1 <= n_agents <= 8");
    if (C.n_beams < 2 || C.theta_dis < 2 || H <= 0 || W <= 0 || !(resolution > 0))
        return fail(F110_E_INVALID, "f110_create: bad sensor/map dimensions");
    if ((uint64_t)(H + 3) * (uint64_t)(W + 3) * 8u >= (1ull << 32))
        return fail(F110_E_INVALID, "f110_create: map too large (the EDT tables are addressed by 32-bit byte offsets)");
    if (!(C.fov > 0) || !(C.fov < 2 * kPi))
        return fail(F110_E_INVALID, "f110_create: fov must be in (0, 2*pi) (one index wrap per scan)");
    if (max_beam_runs((double)C.theta_dis * (C.fov / (double)(C.n_beams - 1)) / (2. * kPi), C.theta_dis) > kMaxSeg)
        return fail(F110_E_INVALID, "f110_create: theta_dis / (fov / n_beams) too large for the beam-index runs "
                                    "(f110_beam_runs.h max_beam_runs <= 80)");
    if (C.ego_idx < 0 || C.ego_idx >= C.n_agents) return fail(F110_E_INVALID, "f110_create: bad ego_idx");
    if (C.integrator != F110_INTEGRATOR_RK4 && C.integrator != F110_INTEGRATOR_EULER)
        return fail(F110_E_INVALID, "f110_create: Invalid Integrator Specified (base_classes.py:399)");
    if (C.autoreset && (!spawn_poses || n_spawn <= 0))
        return fail(F110_E_INVALID, "f110_create: autoreset needs a spawn pose table");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(F110_E_NODEVICE, "f110_create: no HIP device visible");
    if (device < 0 || device >= ndev) return fail(F110_E_NODEVICE, "f110_create: device index out of range");
    if (!is_gfx950(device)) return fail(F110_E_NODEVICE, "f110_create: device is not gfx950 (MI355X)");
    HIP_TRY(hipSetDevice(device));

    f110_ctx *c = new f110_ctx();
    c->arena.device = device;
    c->cfg = C;
    c->p = *params;
    c->H = H;
    c->W = W;
    c->res = resolution;
    for (int i = 0; i < 3; ++i) c->origin[i] = origin[i];
    c->inc = (double)C.theta_dis * (C.fov / (double)(C.n_beams - 1)) / (2. * kPi);  // laser_models.py:367-368
    c->beam_incr = C.fov / (double)(C.n_beams - 1);
    c->n_spawn = n_spawn;
    // The two environment overrides (A/B), read here and nowhere else.  F110_RAY_KERNEL: 1 k_rays_tiled
    // in flat ray order, 2 chunked, 3 the fixed-point kernels; F110_FX_PAD=0 never builds the padded
    // table (the context then steps with k_rays_fxn on the clamped table, or k_rays_fx).
    if (const char *v = std::getenv("F110_RAY_KERNEL")) {
        const int k = std::atoi(v);
        c->ray_kernel = k >= 2 && k <= 3 ? k : 1;
    }
    bool pad_allowed = true;
    if (const char *v = std::getenv("F110_FX_PAD")) pad_allowed = std::atoi(v) != 0;
    {
        // chunked dispatch order: descending beam chunks (the scan's left edge
        // to its right edge).  Measured against the flat order and five other
        // chunk orders (scripts/chunk_ab.py): fastest at 4096
        // and 8192 envs, 1 and 2 agents.
        const int nch = (C.n_beams + 63) / 64;
        if (nch > kMaxChunks && c->ray_kernel >= 2) c->ray_kernel = 1;
        c->nch = nch;
        for (int i = 0; i < nch && i < kMaxChunks; ++i) c->chunk_order[i] = (uint8_t)(nch - 1 - i);
    }
    // the fixed-point kernels' preconditions, and their row-major table's byte offsets (one padding
    // column / row, a zero cell) stay 32-bit: else the chunked tiled kernel
    if (c->ray_kernel == 3 && (!fx_eligible(H, W, resolution, origin, C.eps, edt_k, c->ray_wpb) ||
                               ((uint64_t)W + 16) / 16 * 16 * ((uint64_t)H + 1) * 8 + 128 >= (1ull << 32)))
        c->ray_kernel = 2;
    const size_t EA = (size_t)C.n_envs * C.n_agents;
    const bool fx_ok = c->ray_kernel == 3;
    c->fx_pad = fx_ok && pad_allowed;
    const RayRules rules = ray_rules((int64_t)EA, (int64_t)EA, 1, c->ray_kernel, c->fx_pad);
    c->fx_ilp = fx_ok ? 2 : 1;  // not rules.lanes: alone, 2 also without the padded table (the 12288-car rule
                                // is f110_set_device_share's)
    c->fx_refill = rules.refill;
    if (!rules.heavy_first) c->heavy_T = 0;

    auto cleanup = [&](int rc) {
        destroy_ctx(c);
        return rc;
    };
#define ALLOC(ptr, n)                                                                              \
    do {                                                                                           \
        hipError_t e_ = c->alloc(&(ptr), (n));                                                     \
        if (e_ != hipSuccess) return cleanup(hip_fail("hipMalloc " #ptr, e_, F110_E_ALLOC));       \
    } while (0)

    c->wt = (W + 3) / 4;
    c->tiles_h = (H + 3) / 4;
    ALLOC(c->sines, (size_t)C.theta_dis);
    ALLOC(c->cosines, (size_t)C.theta_dis);
    ALLOC(c->angles, (size_t)C.n_beams);
    ALLOC(c->beam_cos, (size_t)C.n_beams);
    ALLOC(c->side, (size_t)C.n_beams);
    ALLOC(c->cs2, 2 * (size_t)C.theta_dis);
    ALLOC(c->bs2, 2 * (size_t)C.n_beams);
    ALLOC(c->st, 7 * EA);
    ALLOC(c->sb, 2 * EA);
    ALLOC(c->scnt, EA);
    ALLOC(c->ray0, 3 * EA);
    ALLOC(c->runs, (size_t)kMaxSeg * EA);
    ALLOC(c->nruns, EA);
    if (C.n_agents >= 2) ALLOC(c->geo, (size_t)EA * (C.n_agents - 1));
    {
        // k_agents' hand-off chunk masks: their f32 bearings hold to a beam for coordinates below 1 km
        // (handoff_chunks); a larger map stores every chunk instead
        const double extent = std::max(std::fabs(origin[0]), std::fabs(origin[1])) +
                              1.5 * resolution * (double)std::max(H, W);
        if (C.n_agents >= 2 && 64 % C.n_agents == 0 && extent < 1000.0) ALLOC(c->hmask, (size_t)EA);
    }
    ALLOC(c->scan, EA * (size_t)C.n_beams);
    ALLOC(c->reset_flag, (size_t)C.n_envs);
    ALLOC(c->ttc_hit, EA);
    ALLOC(c->noise_step, (size_t)C.n_envs);
    ALLOC(c->start, 3 * EA);
    ALLOC(c->start_rot, 2 * (size_t)C.n_envs);
    ALLOC(c->toggles, EA);
    ALLOC(c->near_start, EA);
    ALLOC(c->lap_times, EA);
    ALLOC(c->lap_counts, EA);
    ALLOC(c->sim_time, (size_t)C.n_envs);
    ALLOC(c->pending, (size_t)C.n_envs);
    ALLOC(c->episode, (size_t)C.n_envs);
    ALLOC(c->nstep, (size_t)C.n_envs);
    ALLOC(c->ctr, (size_t)kCtrSlots * kCtrStride);
    ALLOC(c->pa, (size_t)C.n_agents);
    if (spawn_poses && n_spawn > 0) ALLOC(c->spawn, (size_t)n_spawn * C.n_agents * 3);
    if (c->ray_kernel >= 2 && c->heavy_T > 0) {
        // up to 1/6 of the waves (measured: ~7% of the waves have a ray longer
        // than 40 lookups and carry ~46% of the wave-iterations)
        const size_t div = 6;  // list capacity = 1/div of the waves
        c->heavy_cap = (int32_t)std::max<size_t>(64, (EA * (size_t)c->nch / div + 3) / 4 * 4);
        ALLOC(c->wcost, EA * (size_t)c->nch);
        ALLOC(c->heavy_list, 2 * (size_t)c->heavy_cap);
        ALLOC(c->heavy_mask, EA);
        ALLOC(c->heavy_count, 2);
    }
#undef ALLOC

    std::vector<double> s(C.theta_dis), co(C.theta_dis), an(C.n_beams), bc(C.n_beams), sd(C.n_beams);
    f110_host_tables(C.theta_dis, C.n_beams, C.fov, params, s.data(), co.data(), an.data(), bc.data(), sd.data());
    c->side_max = -INFINITY;
    for (double v : sd) c->side_max = v > c->side_max ? v : c->side_max;  // NaN-free table (f110_host_tables)
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(c->sines, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->cosines, co.data(), co.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->angles, an.data(), an.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->beam_cos, bc.data(), bc.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->side, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice);
    {
        std::vector<double> cs2(2 * (size_t)C.theta_dis), bs2(2 * (size_t)C.n_beams);
        for (int i = 0; i < C.theta_dis; ++i) {
            cs2[2 * (size_t)i] = co[i];
            cs2[2 * (size_t)i + 1] = s[i];
        }
        for (int i = 0; i < C.n_beams; ++i) {
            bs2[2 * (size_t)i] = sd[i];
            bs2[2 * (size_t)i + 1] = bc[i];
        }
        if (e == hipSuccess) e = hipMemcpy(c->cs2, cs2.data(), cs2.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(c->bs2, bs2.data(), bs2.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    c->agent_p.assign((size_t)C.n_agents, *params);
    if (e == hipSuccess)
        e = hipMemcpy(c->pa, c->agent_p.data(), c->agent_p.size() * sizeof(f110_params), hipMemcpyHostToDevice);
    if (e == hipSuccess && c->spawn)
        e = hipMemcpy(c->spawn, spawn_poses, (size_t)n_spawn * C.n_agents * 3 * sizeof(double),
                      hipMemcpyHostToDevice);
    // PAD: the clamp-free loop on a table padded by the max range (+ 8 cells of margin), which
    // k_rays_fxs needs (its offsets, kFxsBase)
    const double pad_q = std::ceil(C.max_range / resolution) + 8.0;
    const int32_t fx_pad_cells = pad_q > 0.0 && pad_q < 65536.0 ? (int32_t)pad_q : 0;  // else no padded table
    if (e == hipSuccess)
        e = acquire_map_tables(device, edt_k, H, W, resolution, c->wt, c->tiles_h, fx_ok,
                               c->fx_pad ? fx_pad_cells : 0, &c->maps);
    if (e == hipSuccess) {
        c->dt = c->maps->dt;
        c->dt_tiled = c->maps->dt_tiled;
        if (fx_ok) {
            c->rm = FxTable{c->maps->rm, c->maps->rm_w, 0, c->maps->rm_oob, c->maps->rm_zero};
            if (c->fx_pad) adopt_padded_table(c);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return cleanup(hip_fail("f110_create upload", e));
    *out = c;
    return F110_OK;
}

extern "C" int f110_destroy(f110_ctx *ctx) {
    if (ctx) destroy_ctx(ctx);
    return F110_OK;
}

// ---------------------------------------------------- the per-step path ----
static TiledMapView tiled_view(const f110_ctx *c) { return make_tiled_view(map_view(c), c->dt_tiled); }

// The context state plan_ray_launch reads, for a step (heavy-first runs its list) or a reset.
RayKnobs ray_knobs(const f110_ctx *c, bool step) {
    const TiledMapView t = tiled_view(c);
    RayKnobs k{};
    k.kernel = c->ray_kernel;
    k.lanes = c->fx_ilp;
    k.refill = c->fx_refill;
    k.fxs_lds = c->fxs_lds;
    k.count_slots = c->count_slots;
    k.wtrace = c->wtrace_armed;
    k.heavy_list = c->wcost != nullptr;
    k.heavy_on = !c->heavy_off;
    k.heavy_use = step && c->wcost && c->ray_kernel >= 2 && !c->heavy_off;
    k.heavy_cap = c->heavy_cap;
    k.has_rm = c->rm.dt != nullptr;
    k.has_rmp = c->rmp.dt != nullptr;
    k.fxs_ok = fxs_ok(c);
    k.rotated = !(t.os == 0.0 && t.oc == 1.0);
    k.E = c->cfg.n_envs;
    k.A = c->cfg.n_agents;
    k.B = c->cfg.n_beams;
    k.theta_dis = c->cfg.theta_dis;
    k.ray_wpb = c->ray_wpb;
    k.has_geo = c->geo != nullptr;
    return k;
}

static StepArgs make_step_args(f110_ctx *c, const f110_outputs *out) {
    StepArgs a{};
    a.map = map_view(c);
    a.tmap = tiled_view(c);
    a.sines = c->sines;
    a.cosines = c->cosines;
    a.angles = c->angles;
    a.beam_cos = c->beam_cos;
    a.side = c->side;
    a.cs2 = c->cs2;
    a.bs2 = c->bs2;
    a.p = c->p;
    a.E = c->cfg.n_envs;
    a.A = c->cfg.n_agents;
    a.B = c->cfg.n_beams;
    a.theta_dis = c->cfg.theta_dis;
    a.integrator = c->cfg.integrator;
    a.ego = c->cfg.ego_idx;
    a.autoreset = c->cfg.autoreset;
    a.fov = c->cfg.fov;
    a.eps = c->cfg.eps;
    a.max_range = c->cfg.max_range;
    a.dt = c->cfg.time_step;
    a.lidar_dist = c->cfg.lidar_dist;
    a.ttc_thresh = c->cfg.ttc_thresh;
    a.side_max = c->side_max;
    a.noise_std = c->cfg.noise_std;
    a.inc = c->inc;
    a.beam_incr = c->beam_incr;
    a.seed = c->cfg.seed;
    a.env_offset = c->cfg.env_offset;
    a.st = c->st;
    a.sb = c->sb;
    a.scnt = c->scnt;
    a.start = c->start;
    a.start_rot = c->start_rot;
    a.toggles = c->toggles;
    a.near_start = c->near_start;
    a.lap_times = c->lap_times;
    a.lap_counts = c->lap_counts;
    a.sim_time = c->sim_time;
    a.pending = c->pending;
    a.episode = c->episode;
    a.nstep = c->nstep;
    a.ray0 = c->ray0;
    a.runs = c->runs;
    a.nruns = c->nruns;
    a.geo = c->geo;
    a.hmask = (c->hcheck & 2) ? nullptr : c->hmask;  // f110_debug_set_handoff_check bit 1: every chunk stored
    a.hcheck = c->hcheck & 5;
    a.scan = c->scan;
    a.reset_flag = c->reset_flag;
    a.ttc_hit = c->ttc_hit;
    a.noise_step = c->noise_step;
    a.noise_ext = c->noise_ext;
    a.pa = c->pa;
    a.spawn = c->spawn;
    a.n_spawn = c->n_spawn;
    if (out) a.out = *out;
    a.ctr = c->ctr;
    a.ray_nch = c->fx_ilp > 1 ? (c->nch + c->fx_ilp - 1) / c->fx_ilp : c->nch;  // k_rays_fxn: chunk groups
    a.parity = (int32_t)(c->launch_n++ & 1);
    if (c->wcost) {
        a.wcost = c->wcost;
        a.heavy_list = c->heavy_list;
        a.heavy_mask = c->heavy_mask;
        a.heavy_count = c->heavy_count;
        a.heavy_cap = c->heavy_cap;
        a.heavy_T = c->heavy_T;
    }
    a.reset_f32 = c->reset_f32 ? 1 : 0;
    if (c->ptab_on) {
        a.ptab = c->ptab;
        a.prange = c->prange_on ? c->prange : nullptr;
        a.pseed = c->pseed;
    }
    if (c->max_steps || c->stall_steps) {
        a.max_steps = c->max_steps;
        a.stall_speed = c->stall_speed;
        a.stall_steps = c->stall_steps;
        a.stall = c->stall_steps ? c->stall : nullptr;
        a.truncated = c->truncated;
    }
    if (c->spawn_on) {
        a.srange = c->srange;
        a.spawn_state = c->spawn_state;
        a.sseed = c->sseed;
    }
    return a;
}

// What the launch reads beside StepArgs; a step's or a reset's (ray_knobs)
static RayLaunch ray_launch(f110_ctx *c, bool step) {
    RayLaunch r{};
    r.k = ray_knobs(c, step);
    r.rm = c->rm;
    r.rmp = c->rmp;
    for (int i = 0; i < kMaxChunks; ++i) r.chunk_order[i] = c->chunk_order[i];
    r.gate_wait = c->gate_wait;
    r.gate_record = c->gate_record;
    if (c->wtrace_armed) {  // one traced ray launch
        r.wtrace = c->wtrace;
        c->wtrace_armed = false;
    }
    return r;
}

extern "C" int f110_reset(f110_ctx *ctx, const double *poses, const uint8_t *env_mask, const f110_outputs *out,
                          void *stream) {
    if (!ctx || !poses) return fail(F110_E_INVALID, "f110_reset: null argument");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    if (out && out->obs_stride && out->obs_stride < (int64_t)ctx->cfg.n_beams + 4 * ctx->cfg.n_agents)
        return fail(F110_E_INVALID, "f110_reset: obs_stride < n_beams + 4*n_agents");
    const RayLaunch r = ray_launch(ctx, /*step=*/false);
    StepArgs a = make_step_args(ctx, out);
    a.mode = 1;
    a.reset_poses = poses;
    a.reset_mask = env_mask;
    HIP_TRY(launch_env_step(a, r, (hipStream_t)stream, ctx->next_prof_events()));
    return F110_OK;
}

static int step_n(f110_ctx *ctx, const void *actions, int32_t actions_dtype, int32_t n, int64_t step_stride,
                  const f110_outputs *out, void *stream, const char *who) {
    if (!ctx || !actions) return fail(F110_E_INVALID, std::string(who) + ": null argument");
    if (actions_dtype != F110_F32 && actions_dtype != F110_F64)
        return fail(F110_E_INVALID, std::string(who) + ": actions_dtype must be F110_F32 or F110_F64");
    if (n < 1) return fail(F110_E_INVALID, std::string(who) + ": n_steps must be >= 1");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    if (out && out->obs_stride && out->obs_stride < (int64_t)ctx->cfg.n_beams + 4 * ctx->cfg.n_agents)
        return fail(F110_E_INVALID, std::string(who) + ": obs_stride < n_beams + 4*n_agents");
    const RayLaunch r = ray_launch(ctx, /*step=*/true);
    StepArgs a = make_step_args(ctx, out);
    a.mode = 0;
    a.heavy_build = r.k.heavy_use;  // k_agents builds the list this step's ray launch runs
    const int64_t packed = (int64_t)ctx->cfg.n_envs * ctx->cfg.n_agents * 2;  // action elements per step
    if (step_stride != 0 && step_stride < packed)
        return fail(F110_E_INVALID, std::string(who) + ": step_stride < n_envs * n_agents * 2");
    const int64_t stride = step_stride ? step_stride : packed;
    for (int32_t t = 0; t < n; ++t) {
        if (actions_dtype == F110_F64)
            a.actions_f64 = static_cast<const double *>(actions) + (size_t)t * stride;
        else
            a.actions = static_cast<const float *>(actions) + (size_t)t * stride;
        if (t) a.parity = (int32_t)(ctx->launch_n++ & 1);
        HIP_TRY(launch_env_step(a, r, (hipStream_t)stream, ctx->next_prof_events()));
    }
    return F110_OK;
}

extern "C" int f110_step(f110_ctx *ctx, const void *actions, int32_t actions_dtype, const f110_outputs *out,
                         void *stream) {
    return step_n(ctx, actions, actions_dtype, 1, 0, out, stream, "f110_step");
}

extern "C" int f110_step_n(f110_ctx *ctx, const void *actions, int32_t actions_dtype, int32_t n_steps,
                           int64_t step_stride, const f110_outputs *out, void *stream) {
    return step_n(ctx, actions, actions_dtype, n_steps, step_stride, out, stream, "f110_step_n");
}

// ------------------------------------------------------ setters / getters --
extern "C" int f110_set_reset_dtype(f110_ctx *ctx, int32_t dtype) {
    if (!ctx || (dtype != F110_F32 && dtype != F110_F64))
        return fail(F110_E_INVALID, "f110_set_reset_dtype: null context or dtype not F110_F32 / F110_F64");
    ctx->reset_f32 = dtype == F110_F32;
    return F110_OK;
}

extern "C" int f110_set_scan_noise(f110_ctx *ctx, const double *noise) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_scan_noise: null context");
    ctx->noise_ext = noise;
    return F110_OK;
}

// For a caller that splits one GPU's cars over several concurrent contexts (streams.StreamShards):
// f110_create's size rules (ray_rules) applied to the cars the device traces at once.
extern "C" int f110_set_device_share(f110_ctx *ctx, int64_t device_cars, int32_t contexts) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_device_share: null context");
    const int64_t own = (int64_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    if (contexts < 1 || device_cars < own)
        return fail(F110_E_INVALID, "f110_set_device_share: contexts >= 1 and device_cars >= this context's cars");
    if (ctx->launch_n != 0) return fail(F110_E_INVALID, "f110_set_device_share: call before the first reset/step");
    const RayRules r = ray_rules(own, device_cars, contexts, ctx->ray_kernel, ctx->fx_pad);
    if (!r.heavy_first) ctx->heavy_off = true;
    if (ctx->ray_kernel != 3) return F110_OK;
    ctx->fx_ilp = r.lanes;
    ctx->fxs_lds = r.fxs_lds;
    return f110_debug_set_ray_refill(ctx, r.refill);  // with the padded table, see there
}

extern "C" int f110_get_state(f110_ctx *ctx, double *state, double *steer_buf, int32_t *steer_cnt, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_get_state: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const size_t EA = (size_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    hipStream_t s = (hipStream_t)stream;
    if (state) HIP_TRY(hipMemcpyAsync(state, ctx->st, 7 * EA * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (steer_buf) HIP_TRY(hipMemcpyAsync(steer_buf, ctx->sb, 2 * EA * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (steer_cnt) HIP_TRY(hipMemcpyAsync(steer_cnt, ctx->scnt, EA * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return F110_OK;
}

extern "C" int f110_get_lap_state(f110_ctx *ctx, double *start_rot, int32_t *toggles, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_get_lap_state: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const size_t E = (size_t)ctx->cfg.n_envs, EA = E * ctx->cfg.n_agents;
    hipStream_t s = (hipStream_t)stream;
    if (start_rot) HIP_TRY(hipMemcpyAsync(start_rot, ctx->start_rot, 2 * E * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (toggles) HIP_TRY(hipMemcpyAsync(toggles, ctx->toggles, EA * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return F110_OK;
}

extern "C" int f110_set_state(f110_ctx *ctx, const double *state, const double *steer_buf, const int32_t *steer_cnt,
                              void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_state: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const size_t EA = (size_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    hipStream_t s = (hipStream_t)stream;
    if (state) HIP_TRY(hipMemcpyAsync(ctx->st, state, 7 * EA * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (steer_buf) HIP_TRY(hipMemcpyAsync(ctx->sb, steer_buf, 2 * EA * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (steer_cnt) HIP_TRY(hipMemcpyAsync(ctx->scnt, steer_cnt, EA * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return F110_OK;
}

// ------------------------------------------------ context-bound batch calls --
extern "C" int f110_scan_batch(f110_ctx *ctx, const double *poses, int64_t M, double *scans, int32_t *lookups,
                               int32_t *hit_rc, void *stream) {
    if (!ctx || !poses || !scans || M < 0) return fail(F110_E_INVALID, "f110_scan_batch: bad arguments");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    ScanArgs a{};
    a.map = map_view(ctx);
    a.sines = ctx->sines;
    a.cosines = ctx->cosines;
    a.B = ctx->cfg.n_beams;
    a.theta_dis = ctx->cfg.theta_dis;
    a.fov = ctx->cfg.fov;
    a.eps = ctx->cfg.eps;
    a.max_range = ctx->cfg.max_range;
    a.inc = ctx->inc;
    a.poses = poses;
    a.M = M;
    a.scans = scans;
    a.lookups = lookups;
    a.hit_rc = hit_rc;
    a.ctr = ctx->ctr;
    HIP_TRY(launch_scan_batch(a, (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_dynamics_batch(f110_ctx *ctx, const double *x, const double *u, double *f, int64_t M,
                                   void *stream) {
    if (!ctx || !x || !u || !f || M < 0) return fail(F110_E_INVALID, "f110_dynamics_batch: bad arguments");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    HIP_TRY(launch_dynamics_batch(x, u, f, M, ctx->p, (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_dynamics_ks_batch(f110_ctx *ctx, const double *x, const double *u, double *f, int64_t M,
                                      void *stream) {
    if (!ctx || !x || !u || !f || M < 0) return fail(F110_E_INVALID, "f110_dynamics_ks_batch: bad arguments");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    HIP_TRY(launch_dynamics_ks_batch(x, u, f, M, ctx->p, (hipStream_t)stream));
    return F110_OK;
}

// ------------------------------------------------------- vehicle params ----
extern "C" int f110_set_params(f110_ctx *ctx, const f110_params *params, int32_t agent_idx, void *stream) {
    if (!ctx || !params) return fail(F110_E_INVALID, "f110_set_params: null argument");
    if (agent_idx >= ctx->cfg.n_agents)  // Simulator.update_params raises IndexError (base_classes.py:544-546)
        return fail(F110_E_INVALID, "f110_set_params: Index given is out of bounds for list of agents.");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    for (int i = 0; i < ctx->cfg.n_agents; ++i)
        if (agent_idx < 0 || i == agent_idx) ctx->agent_p[(size_t)i] = *params;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(ctx->pa, ctx->agent_p.data(), ctx->agent_p.size() * sizeof(f110_params),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // agent_p may change again before an async copy would have read it
    return F110_OK;
}

// The table (allocated on first use, kept until f110_destroy) filled with row(g), car g's f110_params.
template <class Row>
static int upload_param_table(f110_ctx *ctx, hipStream_t s, Row row) {
    const size_t EA = (size_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    if (!ctx->ptab) {
        hipError_t e = ctx->alloc(&ctx->ptab, (size_t)kDynFields * EA);
        if (e != hipSuccess) return hip_fail("hipMalloc ptab", e, F110_E_ALLOC);
    }
    std::vector<double> t((size_t)kDynFields * EA);
    for (size_t g = 0; g < EA; ++g)
        for (int k = 0; k < kDynFields; ++k) t[(size_t)k * EA + g] = fields(row(g))[k];
    HIP_TRY(hipMemcpyAsync(ctx->ptab, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // t goes out of scope
    return F110_OK;
}

extern "C" int f110_set_env_params(f110_ctx *ctx, const f110_params *params, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_env_params: null context");
    if (!params) {  // back to the per-agent params (the randomization redraws table rows: off with it)
        ctx->ptab_on = ctx->prange_on = false;
        return F110_OK;
    }
    const size_t E = (size_t)ctx->cfg.n_envs, A = (size_t)ctx->cfg.n_agents, EA = E * A;
    for (size_t g = 0; g < EA; ++g) {
        const int rc = check_param_row("f110_set_env_params", params[g], ctx->agent_p[g % A], [&] {
            return " (env " + std::to_string(g / A) + ", agent " + std::to_string(g % A) + ")";
        });
        if (rc != F110_OK) return rc;
    }
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const int rc = upload_param_table(ctx, (hipStream_t)stream, [&](size_t g) -> const f110_params & { return params[g]; });
    if (rc == F110_OK) ctx->ptab_on = true;
    return rc;
}

extern "C" int f110_get_env_params(f110_ctx *ctx, f110_params *out, void *stream) {
    if (!ctx || !out) return fail(F110_E_INVALID, "f110_get_env_params: null argument");
    const size_t E = (size_t)ctx->cfg.n_envs, A = (size_t)ctx->cfg.n_agents, EA = E * A;
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<double> t;
    if (ctx->ptab_on) {
        t.resize((size_t)kDynFields * EA);
        HIP_TRY(hipMemcpyAsync(t.data(), ctx->ptab, t.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t g = 0; g < EA; ++g) {
        out[g] = ctx->agent_p[g % A];
        if (ctx->ptab_on)
            for (int k = 0; k < kDynFields; ++k) reinterpret_cast<double *>(&out[g])[k] = t[(size_t)k * EA + g];
    }
    return F110_OK;
}

extern "C" int f110_set_param_randomization(f110_ctx *ctx, const f110_params *lo, const f110_params *hi, uint64_t seed,
                                            void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_param_randomization: null context");
    if (!lo && !hi) {  // off; the table stays as it stands
        ctx->prange_on = false;
        return F110_OK;
    }
    const int A = ctx->cfg.n_agents;
    const int rc = check_param_ranges("f110_set_param_randomization", lo, hi, ctx->agent_p.data(), A);
    if (rc != F110_OK) return rc;  // (before any device call)
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (!ctx->prange) {
        hipError_t e = ctx->alloc(&ctx->prange, (size_t)A * 2 * kDynFields);
        if (e != hipSuccess) return hip_fail("hipMalloc prange", e, F110_E_ALLOC);
    }
    if (!ctx->ptab_on) {  // no table in force: one of the per-agent params
        const int rt = upload_param_table(ctx, s, [&](size_t g) -> const f110_params & { return ctx->agent_p[g % (size_t)A]; });
        if (rt != F110_OK) return rt;
    }
    std::vector<double> r((size_t)A * 2 * kDynFields);
    for (int i = 0; i < A; ++i)
        for (int k = 0; k < kDynFields; ++k) {
            r[((size_t)i * 2) * kDynFields + k] = fields(lo[i])[k];
            r[((size_t)i * 2 + 1) * kDynFields + k] = fields(hi[i])[k];
        }
    HIP_TRY(hipMemcpyAsync(ctx->prange, r.data(), r.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    ctx->pseed = seed;
    ctx->ptab_on = ctx->prange_on = true;
    return F110_OK;
}

// ---------------------------------------------------- spawn randomization --
extern "C" int f110_set_spawn_randomization(f110_ctx *ctx, const f110_spawn_range *ranges, uint64_t seed, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_spawn_randomization: null context");
    if (!ranges) {  // off; the buffers stay
        ctx->spawn_on = false;
        return F110_OK;
    }
    const int A = ctx->cfg.n_agents;
    const int rc = check_spawn_ranges("f110_set_spawn_randomization", ranges, A, ctx->n_spawn);
    if (rc != F110_OK) return rc;  // (before any device call)
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (!ctx->srange) {
        hipError_t e = ctx->alloc(&ctx->srange, (size_t)A);
        if (e == hipSuccess) e = ctx->alloc(&ctx->spawn_state, (size_t)4 * ctx->cfg.n_envs * A);  // (zero-filled)
        if (e != hipSuccess) return hip_fail("hipMalloc spawn ranges", e, F110_E_ALLOC);
    }
    HIP_TRY(hipMemcpyAsync(ctx->srange, ranges, (size_t)A * sizeof(f110_spawn_range), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the caller's array may go away
    ctx->sseed = seed;
    ctx->spawn_on = true;
    return F110_OK;
}

extern "C" int f110_get_spawn_state(f110_ctx *ctx, double *out, void *stream) {
    if (!ctx || !out) return fail(F110_E_INVALID, "f110_get_spawn_state: null argument");
    if (!ctx->spawn_state)
        return fail(F110_E_INVALID, "f110_get_spawn_state: f110_set_spawn_randomization was never turned on");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const size_t EA = (size_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    HIP_TRY(hipMemcpyAsync(out, ctx->spawn_state, 4 * EA * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return F110_OK;
}

// --------------------------------------------------------- episode limits --
extern "C" int f110_set_episode_limits(f110_ctx *ctx, int64_t max_steps, double stall_speed, int32_t stall_steps,
                                       uint8_t *truncated, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_set_episode_limits: null context");
    const int rc = check_episode_limits("f110_set_episode_limits", max_steps, stall_speed, stall_steps);
    if (rc != F110_OK) return rc;  // (before any device call)
    const bool on = max_steps || stall_steps;
    if (stall_steps && !ctx->stall_steps) {  // the stall limit comes on: every env's counter starts at 0
        if (use_device(ctx) != F110_OK) return F110_E_HIP;
        hipStream_t s = (hipStream_t)stream;
        if (!ctx->stall) {
            hipError_t e = ctx->alloc(&ctx->stall, (size_t)ctx->cfg.n_envs);  // (zero-filled)
            if (e != hipSuccess) return hip_fail("hipMalloc stall", e, F110_E_ALLOC);
        } else {
            HIP_TRY(hipMemsetAsync(ctx->stall, 0, (size_t)ctx->cfg.n_envs * sizeof(int32_t), s));
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    ctx->max_steps = max_steps;
    ctx->stall_speed = stall_speed;
    ctx->stall_steps = stall_steps;
    ctx->truncated = on ? truncated : nullptr;
    return F110_OK;
}
