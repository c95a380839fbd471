// f110_ctx.h — the simulator context and the shared map tables (private), for f110_ctx.cpp (create /
// destroy, the per-step path, the setters) and f110_ctx_debug.cpp (the diagnostics).
#pragma once

#include <string>
#include <vector>

#include "../../include/f110.h"
#include "f110_beam_runs.h"
#include "f110_host_util.h"
#include "f110_step_args.h"

// The EDT tables (row-major dt, the 4x4-tiled copy, the fixed-point kernel's
// padded row-major table) are read-only after f110_create.  Contexts on one
// device built from the same map (same H, W, resolution and EDT) share one
// copy: S stream sub-shards of a GPU's envs (streams.StreamShards) then keep
// one table's neighbourhood in each XCD's L2 instead of S (32 MB per copy of
// the Spielberg table).  Refcounted; F110_SHARE_MAP=0 gives each context its
// own copy (A/B).
struct MapTables {
    f110::DeviceArena arena;  // the four tables
    int32_t H = 0, W = 0;
    uint64_t res_bits = 0;
    std::vector<uint32_t> k;  // the EDT the tables were built from (exact match, not a hash)
    const double *dt = nullptr, *dt_tiled = nullptr, *rm = nullptr, *rmp = nullptr;
    int32_t rm_w = 0, rmp_w = 0, rmp_P = 0, rmp_h = 0;
    uint32_t rm_oob = 0, rm_zero = 0, rmp_zero = 0;
    int refs = 0;
    bool shared = true;
};

struct f110_ctx {
    f110::DeviceArena arena;    // every device buffer below but the map tables
    MapTables *maps = nullptr;  // the shared read-only EDT tables (dt, dt_tiled, rm)
    f110_config cfg{};
    f110_params p{};                 // Simulator-level params (fixed at create)
    std::vector<f110_params> agent_p;  // RaceCar params per agent (f110_set_params)
    f110_params *pa = nullptr;       // device copy of agent_p
    int H = 0, W = 0;
    double res = 0, origin[3] = {0, 0, 0};
    double inc = 0, beam_incr = 0;
    int n_spawn = 0;
    // device buffers
    const double *dt_tiled = nullptr;
    int32_t wt = 0, tiles_h = 0;
    int ray_kernel = 3;  // F110_RAY_KERNEL: 1 tiled flat order, 2 tiled chunked, 3 the fixed-point
                         // kernels (default; falls back to 2 where their preconditions fail)
    uint8_t chunk_order[f110::kMaxChunks] = {};
    const double *dt = nullptr;
    double *sines = nullptr, *cosines = nullptr, *angles = nullptr, *beam_cos = nullptr, *side = nullptr,
           *spawn = nullptr;
    double *cs2 = nullptr, *bs2 = nullptr;  // interleaved (cos, sin)[theta_dis], (side, beam_cos)[B] (k_rays_fxs)
    double side_max = 0.0;                  // max of the side table (k_rays_fxs's TTC pre-test)
    double *start_rot = nullptr;
    double *st = nullptr, *sb = nullptr, *start = nullptr, *sim_time = nullptr, *ray0 = nullptr, *scan = nullptr;
    f110::BeamRun *runs = nullptr;
    int32_t *nruns = nullptr;
    f110::PairGeom *geo = nullptr;  // [E][A][A-1] ray_cast pair geometry (A >= 2)
    uint32_t *hmask = nullptr;  // [E*A] hand-off chunk masks of k_rays_fxs<HANDOFF> (A >= 2 dividing 64)
    uint64_t *noise_step = nullptr;
    int32_t *scnt = nullptr, *toggles = nullptr;
    uint8_t *near_start = nullptr, *pending = nullptr, *reset_flag = nullptr, *ttc_hit = nullptr;
    float *lap_times = nullptr, *lap_counts = nullptr;
    uint64_t *episode = nullptr, *nstep = nullptr;
    unsigned long long *ctr = nullptr;
    // f110_profile_begin/end
    std::vector<hipEvent_t> prof_ev;  // 6 per recorded step: (start, stop) of k_agents, the ray kernel, k_post
    int prof_max = 0, prof_n = 0;
    const double *noise_ext = nullptr;  // f110_set_scan_noise (caller-owned)
    uint64_t *wtrace = nullptr;         // f110_debug_wave_trace buffer (diagnostics)
    bool heavy_off = false;             // f110_debug_disable_heavy_first
    bool reset_f32 = false;             // f110_set_reset_dtype
    hipEvent_t gate_wait = nullptr;     // f110_debug_set_ray_gate (caller-owned events)
    hipEvent_t gate_record = nullptr;
    // heavy-first ray dispatch (chunked kernel)
    uint8_t *wcost = nullptr;
    uint32_t *heavy_list = nullptr, *heavy_mask = nullptr, *heavy_count = nullptr;
    int32_t heavy_cap = 0, heavy_T = 16, nch = 0;  // with one-wave blocks and a 1/6 list: 16 best
    uint64_t launch_n = 0;
    int ray_wpb = 1;  // one-wave blocks (4-car blocks measured slower)
    int64_t wtrace_n = 0;
    bool wtrace_armed = false;
    f110::FxTable rm{}, rmp{};  // the fixed-point kernels' clamped and padded EDT (shared, see MapTables)
    int32_t rmp_h = 0;    // rows of the padded table
    bool fx_pad = false;    // the padded table may be built (the fixed-point kernels, unless F110_FX_PAD=0 at create)
    int32_t fx_refill = 0;   // waves per car of k_rays_fxs (0 = k_rays_fxn; f110_debug_set_ray_refill)
    bool fxs_lds = false;    // single-agent k_rays_fxs with the LDS theta table (f110_set_device_share, > 1 context)
    bool count_slots = false;  // f110_debug_set_simt: lane-slot counter of the fixed-point loops (f110_debug_read_simt)
    int32_t hcheck = 0;        // f110_debug_set_handoff_check: bit 0 poison + count misses, bit 1 mask off,
                               // bit 2 an empty mask (the check's own test)
    int fx_ilp = 1;         // rays per lane (f110_debug_set_ray_lanes; default by car count)
    // per-env vehicle params (f110_set_env_params / f110_set_param_randomization); the buffers are
    // allocated by the first setter that needs them and kept until f110_destroy
    double *ptab = nullptr;    // [kDynFields][E*A]
    double *prange = nullptr;  // [A][2][kDynFields]
    bool ptab_on = false, prange_on = false;  // the steps read the table / redraw rows at resets
    uint64_t pseed = 0;
    // episode limits (f110_set_episode_limits); stall: [E], allocated by the first stall limit
    int64_t max_steps = 0;
    double stall_speed = 0.0;
    int32_t stall_steps = 0;
    int32_t *stall = nullptr;
    uint8_t *truncated = nullptr;  // caller-owned
    // spawn randomization (f110_set_spawn_randomization); both buffers are allocated by the first
    // call that turns it on and kept until f110_destroy
    f110_spawn_range *srange = nullptr;  // [A]
    double *spawn_state = nullptr;       // [4][E*A]
    bool spawn_on = false;               // resetting cars draw their start state
    uint64_t sseed = 0;

    hipEvent_t *next_prof_events() {
        if (prof_n >= prof_max) return nullptr;
        return &prof_ev[(size_t)6 * prof_n++];
    }
    void free_prof() {
        for (hipEvent_t e : prof_ev) (void)hipEventDestroy(e);
        prof_ev.clear();
        prof_max = prof_n = 0;
    }

    // a zero-filled buffer of n elements (16 bytes when n is 0)
    template <class T>
    hipError_t alloc(T **p, size_t n) {
        return arena.alloc(p, n, /*zero=*/true, 0, 16);
    }
};

// ---- f110_ctx.cpp, for the debug surface ----------------------------------------
int use_device(const f110_ctx *c);                       // makes the context's device current
f110::RayKnobs ray_knobs(const f110_ctx *c, bool step);  // the context state plan_ray_launch reads
int ensure_padded_table(f110_ctx *ctx);                  // the padded EDT k_rays_fxs needs, built on first use
