// f110_step_args.h — the env step's kernel argument blocks (StepArgs, RayArgs), the fixed-point
// constants of the ray kernels, the ray launch's plan and the launchers of the step's stages,
// shared by the step's .hip files (device) and the context (f110_ctx.cpp, f110_step.cpp).
// Host-only helpers are in f110_host_util.h (errors, DeviceArena) and f110_host.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_beam_runs.h"
#include "f110_map.h"

namespace f110 {

// Lookup/ray counters are spread over kCtrSlots 128-B lines: ~10^5 waves
// adding into ONE address serialise at the memory side (measured: 2.7 ms of
// a 3.4 ms scan at 8192 envs); 256 slots make the adds contention-free.
constexpr int kCtrSlots = 256;
constexpr int kCtrStride = 16;  // u64 per slot (128 B)
constexpr int kRayBlock = 256; // threads per block of the ray kernels
constexpr int kMaxMultiBodies = 64;  // f110_collision_multiple: bodies per set
constexpr int kMaxChunks = 32;  // 64-beam chunks per scan (n_beams <= 2048) for the chunked ray dispatch

// What the kernels of one env step (k_agents, the post kernels) read, passed by value; what only the
// host reads to launch them travels beside it (RayLaunch below).
struct PairGeom;  // below

struct StepArgs {
    MapView map;
    TiledMapView tmap;
    const double *sines, *cosines;            // [theta_dis]  ScanSimulator2D tables
    const double *angles, *beam_cos, *side;   // [B] RaceCar class-level beam tables
    const double *cs2, *bs2;  // k_rays_fxs: (cos, sin)[theta_dis], (side, beam_cos)[B] interleaved
    f110_params p;                            // Simulator / F110Env params (GJK boxes, lidar_max)
    const f110_params *pa;                    // [A] RaceCar params (update_pose, ray_cast boxes)
    int32_t E, A, B, theta_dis, integrator, ego, autoreset, mode;  // mode 0 step, 1 reset
    int32_t reset_f32;        // resets follow F110Env.reset(options=float32 poses) (f110_set_reset_dtype)
    // heavy-first ray dispatch (chunked kernel): per (car, chunk) wave cost of
    // the previous ray launch, this step's list of predicted-heavy waves
    uint8_t *wcost;           // [EA][nch] min(255, longest ray of the wave) or null
    uint32_t *heavy_list;     // [2][heavy_cap] (car << 8 | chunk), by step parity
    uint32_t *heavy_mask;     // [EA] chunks of the car that are in the heavy list
    uint32_t *heavy_count;    // [2] list lengths, by step parity
    int32_t heavy_cap, heavy_T, heavy_build, parity, ray_nch;
    uint32_t *hmask;    // [E*A] k_agents' hand-off chunk masks (A >= 2 dividing 64), or null
    PairGeom *geo;      // [E][A][A-1] pair geometry (A >= 2), see RayArgs::geo
    int32_t geo_ready;  // set by launch_env_step: this step's ray kernel computed geo
    int32_t hcheck;       // f110_debug_set_handoff_check bit 0: the hand-off buffer is NaN-poisoned before the
                          // ray launch and k_post_multi counts its reads outside hmask (ctr[.][6]); bit 2:
                          // k_agents stores empty masks (a forced miss, the check's own test)
    double fov, eps, max_range, dt, lidar_dist, ttc_thresh, noise_std, inc, beam_incr;
    double side_max;  // max of the RaceCar side table (the TTC pre-test of k_rays_fxs)
    uint64_t seed;
    int64_t env_offset;
    // persistent per-agent / per-env state (SoA, owned by the context)
    double *st;          // [7][E*A]
    double *sb;          // [2][E*A] steer buffer (newest, older)
    int32_t *scnt;       // [E*A]
    double *start;       // [3][E*A] reset poses (lap logic)
    double *start_rot;   // [2][E] cos(-th), sin(-th) of the ego's reset yaw
    int32_t *toggles;    // [E*A]
    uint8_t *near_start; // [E*A]
    float *lap_times;    // [E*A]
    float *lap_counts;   // [E*A]
    double *sim_time;    // [E]
    uint8_t *pending;    // [E] autoreset pending
    uint64_t *episode;   // [E]
    uint64_t *nstep;     // [E] steps since reset (noise counter)
    // k_agents -> k_rays -> k_post hand-off buffers (context scratch)
    double *ray0;        // [3][E*A] scan pose x, y and first EDT lookup d0
    BeamRun *runs;       // [E*A][kMaxSeg] beam-index runs
    int32_t *nruns;      // [E*A]
    double *scan;        // [E*A][B] ranges (noise added) before the collision stage
    uint8_t *reset_flag; // [E] this call reset the env
    uint8_t *ttc_hit;    // [E*A] TTC fired in the fused single-agent ray pass
    uint64_t *noise_step;// [E] noise counter used by this step
    const double *noise_ext;  // [E][B] caller-supplied scan noise (f110_set_scan_noise) or null
    const double *spawn; // [n_spawn][A][3]
    int32_t n_spawn;
    // inputs
    const float *actions;       // [E][A][2] f32, or
    const double *actions_f64;  // [E][A][2] f64
    const double *reset_poses;  // [E][A][3]
    const uint8_t *reset_mask;  // [E] or null
    f110_outputs out;
    unsigned long long *ctr;    // [kCtrSlots][16]: [0] lookups, [1] rays (see count_rays), [2] lane slots of the fixed-point loops
    // per-env vehicle params (f110_set_env_params; last, so that every field above keeps its kernarg offset)
    double *ptab;          // [kDynFields][E*A] the dynamics fields per car (k_agents<., PENV>), or null: a.pa[ag]
    const double *prange;  // [A][2][kDynFields] (lo, hi) a resetting car redraws its row from, or null
    uint64_t pseed;        // f110_set_param_randomization's seed
    // episode limits (f110_set_episode_limits; appended for the same reason).  Both limits 0: the post
    // kernels' epilogue is the limit-free one (no load or store of the fields below)
    int64_t max_steps;     // time limit in steps since the reset (a.nstep's count), 0 = none
    double stall_speed;    // |ego v| below this counts as standing
    int32_t stall_steps;   // standing steps in a row that truncate, 0 = none
    int32_t *stall;        // [E] the stall counters (set when stall_steps != 0)
    uint8_t *truncated;    // [E] the caller's flag buffer, or null
    // spawn randomization (f110_set_spawn_randomization; appended for the same reason)
    const f110_spawn_range *srange;  // [A] the agents' ranges (k_agents<., ., SPAWN>), or null: off
    double *spawn_state;             // [4][E*A] (x, y, yaw, speed) of each car's last drawn reset
    uint64_t sseed;                  // f110_set_spawn_randomization's seed
};

// RN(1 / lidar_max) in f32 for k_rays_fxs's obs division, or 0 (the IEEE
// divide) outside [2^-30, 2^30], where an intermediate could be subnormal
inline float obs_reciprocal(float lmax) {
    if (!(lmax >= 0x1p-30f && lmax <= 0x1p30f)) return 0.0f;
    volatile float l = lmax;  // one IEEE f32 divide (not folded into a double one)
    return 1.0f / l;
}

// f110_agent_obs / f110_host_agent_obs: the argument errors both report as F110_E_INVALID
inline bool agent_obs_bad_args(const float *scans, int64_t scan_env_stride, const float *obs, int64_t obs_stride,
                               int64_t n_envs, int32_t n_agents, int32_t n_beams, int32_t agent, const float *out,
                               int64_t out_stride) {
    if (!scans || !obs || !out || n_envs <= 0 || n_agents <= 0 || n_beams <= 0 || agent < 0 || agent >= n_agents)
        return true;
    const int64_t row = (int64_t)n_beams + 4 * (int64_t)n_agents;
    return scan_env_stride < (int64_t)n_agents * n_beams || obs_stride < row || out_stride < row;
}

// k_rays_tiled's own argument block: only what the ray loop and its epilogue
// read (the full StepArgs kept 90 SGPRs live: 7 instead of 8 blocks per CU).
// One (car, opponent) pair's agent ray_cast geometry (RaceCar.ray_cast_agents,
// base_classes.py:206-227; laser_models.py:282-346): the opponent's box as the
// car sees it (get_vertices with the car's params), the box's beam window at
// the scan origin and the beam-index ranges of the blocked view the window can
// hold.  Computed by the ray kernel's leading geometry blocks (k_rays_fxs with
// other cars in the env) from the post-update, pre-TTC poses; k_post_multi
// recomputes the pairs whose car's TTC fired (its yaw is zeroed).
struct PairGeom {
    double rv[8];
    double phi[4];  // vertex bearings (box_beam_window's input)
    double wc, wh;
    int32_t rng[4];
};

struct RayArgs {
    TiledMapView m;
    const double *sines, *cosines;
    const double *ray0;        // [3][EA]
    const BeamRun *runs;       // [EA][kMaxSeg]
    const int32_t *nruns;      // [EA]
    const uint8_t *reset_mask; // [E]: f110_reset with an env mask, else null
    double *scan;              // [EA][B]
    const double *noise_ext;   // [E][B] or null
    const uint64_t *noise_step;// [E]
    unsigned long long *ctr;
    double eps, max_range, noise_std;
    uint64_t seed;
    int64_t env_offset;
    int32_t EA, A, B, theta_dis;
    // FUSED single-agent epilogue (k_rays_tiled<.., .., true>)
    const double *vel;         // state[3][EA]
    const double *beam_cos, *side;
    double ttc_thresh;
    double side_max;           // max_b side[b]: a range above side_max + 1.2 thresh |v| cannot fire TTC
    uint8_t *ttc_hit;          // [EA]
    float *obs;                // [E][obs_len] or null
    float *scans_f32;          // [EA][B] or null
    double *scans_f64;         // [EA][B] or null
    int32_t obs_len;
    float lidar_max;
    float obs_rinv;            // RN(1 / lidar_max) for k_rays_fxs's obs division (0: IEEE divide)
    // chunked dispatch (k_rays_tiled<.., CH = true>)
    int32_t G4;                // blocks per chunk slot (4 cars per block)
    uint8_t order[kMaxChunks]; // chunk of each slot
    uint64_t *wtrace;          // diagnostic wave trace [waves][4] or null
    // heavy-first dispatch: HB leading blocks run the listed heavy waves
    uint8_t *wcost;            // [EA][nch] written by every chunked launch (or null)
    const uint32_t *heavy_list;
    const uint32_t *heavy_mask;
    const uint32_t *heavy_count;
    int32_t HB, nch;
    int32_t wpb;  // chunked: waves (cars) per block
    // fixed-point cell index of k_rays_fx (see fx_step in f110_rays_fx.h):
    // t = fma(x, inv_res, fx_cx) = 1.5*2^22 + column, on a 2^-30 grid
    double fx_cx, fx_cy;
    // |q| bound of a scan origin whose rays stay in t's binade: 2^21 - 32 - max_range / res
    double fx_lim;
    uint32_t fx_zero;  // byte offset of the row-major table's zero cell (k_rays_fxn)
    // PAD (k_rays_fxn on the padded table): fx_cx / fx_cy = 2^24 + P - origin /
    // res, and a car takes the clamp-free loop when its scan origin's q lies in
    // [fxp_lo, fxp_hx) x [fxp_lo, fxp_hy): every lookup of its rays then lands
    // inside the padded table (see fxp_offset)
    double fxp_lo, fxp_hx, fxp_hy;
    int32_t fxp_P;
    double fxs_cx, fxs_cy;  // k_rays_fxs: 2^20 + P + 2^-26 - origin / res (see kFxsBase)
    int32_t count_slots;  // the fixed-point loops add their lane slots to ctr[.][2] (f110_debug_read_simt)
    const double *cs2, *bs2;  // k_rays_fxs: interleaved (cos, sin) / (side, beam_cos) tables
    // k_rays_fxs<HANDOFF>: geo_blocks leading work items (one wave each) compute every pair's PairGeom
    const uint32_t *hmask;     // [EA] the chunks whose hand-off k_post_multi may read (k_agents), or null: all
    PairGeom *geo;
    int32_t geo_blocks;
    const double *st;          // state [7][EA] after k_agents
    const f110_params *pa;     // [A] per-agent params (RaceCar.params)
    double fov, beam_incr;
};

// k_rays_fx's magic offset: 1.5 * 2^22.  t = M + q for q in [0, 2^21) lies in
// the binade [2^22, 2^23), whose ulp is 2^-30, so the low 30 mantissa bits of
// t hold q's fraction and the next 21 its integer part.
constexpr double kFxMagic = 6291456.0;
// bits [61:30] of M: exponent[9:0] (0x015), mantissa bit 51, 21 zero bits
constexpr uint32_t kFxU0 = 0x05600000u;
// guard band of the fixed-point fraction, in units of 2^-30 (error budget < 2^-29)
constexpr uint32_t kFxBand = 4u;
// PAD: t = fma(x, inv_res, 2^24 + P - origin / res) lies in [2^24, 2^25),
// ulp 2^-28.  Bits [51:28] of t (one v_alignbit by 28) hold int(t) - 2^24 =
// floor(q) + P in their low 24 bits -- exactly the operand a 24-bit multiply
// reads, so the padded table's byte offset is two u24 multiply(-add)s with no
// bias subtraction and no clamp.  Error budget (units of q): the constant's
// and t's roundings (2^-29 each), inv_res's (< 2^-31 for |x / res| < 2^21)
// and the reference's own (< 2^-31): < 2^-27.4; the guard band is kFxpBand *
// 2^-28 = 2^-26.
constexpr double kFxpBase = 16777216.0;
constexpr uint32_t kFxpBand = 4u;
// k_rays_fxs: t = fma(x, inv_res, 2^20 + P + 2^-26 - origin / res) lies in
// [2^20, 2^21), ulp 2^-32: t's low dword is the fraction of q + P + 2^-26 and
// its high dword's low 24 bits are 3 * 2^20 (the exponent's low bits) +
// floor(q + P + 2^-26) -- the u24 multiplies read the high dwords as they are
// (no v_alignbit).  The 3 * 2^20 terms add 3 * 2^20 * (k1 + 8) to the byte
// offset, which vanishes mod 2^32 because the padded table's row stride k1 is
// 8 bytes short of a multiple of 4096 (build_padded_table).  The +2^-26 shift
// makes the guard band one compare: a lane is near a cell edge when the low
// dword is below 2 * kFxsBand (= 2^-25, a band of 2^-26 on either side of the
// edge, as kFxpBand); such lanes take the IEEE cell, so the shifted integer
// part of the others is floor(q + P).  Error budget (units of q): t's and the
// constant's roundings (2^-33 each) and those of kFxpBase's analysis: < 2^-27.4.
constexpr double kFxsBase = 1048576.0;
constexpr double kFxsShift = 0x1p-26;
constexpr uint32_t kFxsBand = 64u;  // 2^-26 in units of 2^-32
constexpr int kFxsWaves = 8;         // k_rays_fxs: work items (one wave each) per block, sharing one LDS theta table
constexpr int kFxsLdsTheta = 2048;   // theta table entries the block's LDS copy holds (32 KB; theta_dis 2000)

// The ray launch of one f110_step / f110_reset, decided in one place: RayKnobs is the context state
// the decision reads (plain values, include/f110_debug.h), RayPlan the kernel family, its template
// flags, the launch shape and the EDT table.  plan_ray_launch (f110_host.cpp) is pure host code: no HIP
// call, no context, no environment (tests/test_host_lib.py checks it on the CPU through f110_host_ray_plan).
using RayKnobs = f110_ray_knobs;
using RayPlan = f110_ray_plan;
RayPlan plan_ray_launch(const RayKnobs &k, bool masked);

// A row-major EDT of the fixed-point kernels: rows of w cells, a 0.0 at byte `zero` past the end.
// The clamped one (k_rays_fx / k_rays_fxn): 128-B aligned rows, columns W..w-1 and row H hold
// dt[-1,-1], oob = byte offset of dt[H-1][W-1], P = 0.  The padded one (k_rays_fxn<PAD> /
// k_rays_fxs): P cells of dt[-1,-1] on every side (cell (r, c) at row r + P, column c + P), oob = 0.
struct FxTable {
    const double *dt;  // null: not built
    int32_t w, P;
    uint32_t oob, zero;
};

// What launch_env_step needs beside StepArgs and no kernel reads through it.
struct RayLaunch {
    RayKnobs k;
    FxTable rm, rmp;                  // the clamped and the padded table
    uint8_t chunk_order[kMaxChunks];  // beam-chunk dispatch order of the chunked kernels
    uint64_t *wtrace;                 // diagnostic wave trace of this ray launch (f110_debug_wave_trace) or null
    hipEvent_t gate_wait;             // f110_debug_set_ray_gate: waited on before the ray launch, or null
    hipEvent_t gate_record;           //   recorded after it, or null
};

// ---- the env step (f110_step.cpp) and its stages, one translation unit each --------------------
hipError_t launch_env_step(const StepArgs &a, const RayLaunch &r, hipStream_t s,
                           hipEvent_t *ev = nullptr);  // ev: 6 events or null
// start / stop: the events of the kernel's own dispatch, or null
hipError_t launch_agents(const StepArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop);  // f110_agents.hip
hipError_t launch_post(const StepArgs &a, bool geo_ready, hipStream_t s, hipEvent_t start,
                       hipEvent_t stop);  // f110_post.hip; geo_ready: the ray launch computed a.geo
// The kernel of a plan of the family: each ray file owns the table of its instantiations, and no
// kernel is referenced from another translation unit except through these.
using RayKernel = void (*)(RayArgs);
RayKernel tiled_ray_kernel(const RayPlan &p);  // f110_rays_tiled.hip
RayKernel fx_ray_kernel(const RayPlan &p);     // f110_rays_fx.hip: k_rays_fx, k_rays_fxn
RayKernel fxs_ray_kernel(const RayPlan &p);    // f110_rays_fxs.hip

}  // namespace f110
