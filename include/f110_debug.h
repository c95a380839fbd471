/*
 * f110_debug.h -- measurement, diagnostics, A/B scheduling knobs and host
 * test hooks of libf110.so (the same shared library as include/f110.h).
 *
 * None of these is part of the drop-in boundary (include/f110.h): the
 * reference has no counterpart for them.  They are used by bench.py, the
 * profiling scripts and the tests.  Results never depend on them: the
 * counters and timers only observe, and the f110_debug_set_* knobs change
 * which ray kernel variant runs, never what it computes (every variant is
 * bit-identical, tests/test_gpu_batch.py).  Conventions as in f110.h.
 */
#ifndef F110_DEBUG_H
#define F110_DEBUG_H

#include "f110.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- counters -------------------------------------------------------------
 * EDT lookups and rays traced by f110_step/f110_reset/f110_scan_batch since
 * the last reset of the counters (device-side accumulation; reading syncs
 * `stream`).  Used for the measured mean lookups per ray (roofline).
 * k_rays_fxs, the default ray kernel of f110_step, counts only while counting
 * is on (f110_debug_set_simt): its uncounted build keeps the per-trip
 * bookkeeping out of the timed loop; the other ray kernels always count. */
F110_API int f110_read_counters(f110_ctx *ctx, uint64_t *lookups, uint64_t *rays, void *stream);
F110_API int f110_reset_counters(f110_ctx *ctx, void *stream);
/* Diagnostic: the sum over the counter lines of counter idx (0..15): 0
 * lookups, 1 rays, 2 lane slots (f110_debug_read_simt). */
F110_API int f110_debug_read_counter(f110_ctx *ctx, int32_t idx, uint64_t *value, void *stream);
/* SIMT efficiency of the fixed-point ray loops (k_rays_fx / k_rays_fxn /
 * k_rays_fxs, the default kernels) since the last counter reset: loop_lookups
 * = lookups made inside the loop (all lookups less the first one per ray,
 * which k_agents makes), lane_slots = 64 x the wave-level gathers the loop
 * issued (k_rays_fx / k_rays_fxn: trip count x rays per lane; k_rays_fxs:
 * trips x 2 slots, a closed slot's zero-cell gather included), summed over
 * waves; efficiency = loop_lookups / lane_slots.  Other ray
 * kernels, and launches made while the count is off, leave lane_slots as
 * they are.  f110_debug_set_simt(ctx, 1) turns the count on (off by default: its
 * extra atomic per wave costs ~2 % of k_rays).  Diagnostics (no reference
 * counterpart).  While it is on, f110_step runs k_rays_fxs's counting build
 * (lookups, rays, lane slots, other loads: counters 0-3 and 5). */
F110_API int f110_debug_set_simt(f110_ctx *ctx, int32_t on);
F110_API int f110_debug_read_simt(f110_ctx *ctx, uint64_t *loop_lookups, uint64_t *lane_slots, void *stream);

/* Hand-off mask check (multi-agent contexts).  k_agents marks, per car, the
 * 64-beam chunks whose f64 scan k_post_multi's agent ray_cast may read, and
 * the ray kernel stores only those chunks into the hand-off buffer.  mode bit
 * 0: before each ray launch the hand-off buffer is filled with NaN and
 * k_post_multi counts every read of a beam whose chunk bit is clear into
 * counter 6 (f110_debug_read_counter); bit 1: no mask (every chunk stored, the
 * reference for bit-identity); bit 2: every mask empty (a forced miss: the
 * check's own test).  0 restores the default.  Debug only: with the
 * mask correct, outputs are the same bits in every mode. */
F110_API int f110_debug_set_handoff_check(f110_ctx *ctx, int32_t mode);

/* ---- per-kernel timing ----------------------------------------------------
 * Attaches a (start, stop) HIP event pair to the dispatch of each of the
 * three kernels of the next max_steps f110_step/f110_reset calls (k_agents,
 * k_rays, k_post; hipExtLaunchKernel: the kernel's own begin / end
 * timestamps, no marker packet between the kernels).
 * f110_profile_end waits for them and returns the summed milliseconds per
 * kernel and the number of steps recorded.  Used by bench.py for the
 * roofline of the dominant kernel (k_rays). */
F110_API int f110_profile_begin(f110_ctx *ctx, int32_t max_steps);
F110_API int f110_profile_end(f110_ctx *ctx, double ms_out[3], int32_t *steps_out);
/* Before f110_profile_end: the recorded steps' six timestamps (begin / end of
 * k_agents, the ray kernel, k_post) in ms after ref_event (a caller-owned
 * hipEvent_t with timing, recorded before those steps on any stream of the
 * device): out[step][6], up to max_steps steps; steps_out gets the count.
 * bench.py takes the union of the ray kernels' intervals over concurrent
 * stream sub-shards from it (the timed runner's own ray time). */
F110_API int f110_debug_profile_stamps(f110_ctx *ctx, void *ref_event, double *out, int32_t max_steps,
                                       int32_t *steps_out);

/* ---- diagnostics -------------------------------------------------------------
 * Wave trace of the ray kernel (one-wave blocks: k_rays_fx / k_rays_fxn /
 * k_rays_fxs, or the chunked k_rays_tiled on an axis-aligned map without a
 * reset mask): arm != 0 records the next f110_step's ray launch -- per wave
 * (block) {start, end} s_memrealtime ticks (100 MHz), {XCC id << 32 | HW_ID},
 * {item << 32 | car} (item: the chunk, chunk group, or k_rays_fxs's trips << 8
 * | wave of the car).  Entries of waves that did not run stay 0.  host_out
 * [max_waves][4] (or NULL) receives the last trace (waits for `stream`);
 * n_waves gets the buffer's capacity in waves. */
F110_API int f110_debug_wave_trace(f110_ctx *ctx, int32_t arm, uint64_t *host_out, int64_t max_waves,
                                   int64_t *n_waves, void *stream);

/* Ray gate for sub-shards stepped on concurrent streams (one context per
 * sub-shard, one stream each).  A non-null wait_event is waited on (stream
 * side) before every following f110_step / f110_reset ray launch of this
 * context; a non-null record_event is recorded right after it.  Chaining
 * the sub-shards' events in a ring keeps their ray passes in order (never two
 * ray grids competing for the CUs) while their k_agents / k_post launches run
 * beside another sub-shard's ray pass.  Events are caller-owned hipEvent_t;
 * NULL, NULL turns the gate off.  Scheduling only: results are unchanged. */
F110_API int f110_debug_set_ray_gate(f110_ctx *ctx, void *wait_event, void *record_event);

/* Turns the heavy-first ray dispatch off for the following f110_step calls of
 * this context (permanent).  Heavy-first starts the previous
 * step's long waves first so one ray grid does not end on them; when another
 * sub-shard's ray pass runs beside this one on a concurrent stream, that
 * tail is filled anyway and the list upkeep is the larger cost.
 * Scheduling only: results are unchanged. */
F110_API int f110_debug_disable_heavy_first(f110_ctx *ctx);

/* The ray kernel this context launches (>= 0), or a negative error code:
 * 1 k_rays_tiled in flat ray order, 2 tiled chunked, 3 the fixed-point
 * kernels k_rays_fx / k_rays_fxn / k_rays_fxs (the default where their
 * preconditions hold: axis-aligned map, EDT entries 0 or > eps).  Selected at
 * f110_create (env F110_RAY_KERNEL overrides the default, A/B only). */
F110_API int f110_debug_ray_kernel(const f110_ctx *ctx);

/* Rays traced per lane by the fixed-point ray kernel (1: k_rays_fx, 2:
 * k_rays_fxn / k_rays_fxs; size-based default, f110_debug_set_ray_lanes); 1 for the
 * other ray kernels.  Diagnostic, no reference counterpart. */
F110_API int f110_debug_ray_lanes(const f110_ctx *ctx);
/* k_rays_fxs's waves per car for unmasked steps (one wave per car traces the
 * car's 64-beam chunks two at a time, refilling a slot as soon as its chunk
 * ends), or 0 when the context steps with k_rays_fxn / k_rays_fx (heavy-first
 * on, one ray per lane, no padded table).  Default: 1 from 32768 cars. */
F110_API int f110_debug_ray_refill(const f110_ctx *ctx);
/* Set k_rays_fxs's waves per car (0: k_rays_fxn) and, when on, switch the
 * context to the padded EDT (built on first use) and off its heavy-first list.
 * For callers that split one GPU's cars over several contexts
 * (streams.StreamShards): the size rule is about the cars the GPU traces at
 * once, not one context's.  Any time.  Scheduling only: results are unchanged. */
F110_API int f110_debug_set_ray_refill(f110_ctx *ctx, int32_t waves);

/* Sets the rays per lane of the fixed-point ray kernel (1 or 2) before the
 * context's first reset/step.  The size-based default looks at this
 * context's cars only; a caller stepping S contexts concurrently on one GPU
 * (streams.StreamShards) knows the GPU's total and passes the choice for
 * that.  Scheduling only: results are unchanged.
 * Diagnostic / tuning, no reference counterpart. */
F110_API int f110_debug_set_ray_lanes(f110_ctx *ctx, int32_t n);

/* ---- the ray launch plan (host) --------------------------------------------
 * Which ray kernel a context launches, on which grid and EDT table, is one
 * pure function of the plain values below (plan_ray_launch in
 * f110_host.cpp): f110_step / f110_reset launch what it
 * returns, and the f110_debug_ray_* getters read it. */
enum { F110_RAY_TILED_FLAT = 0, F110_RAY_TILED_CHUNKED, F110_RAY_FX, F110_RAY_FXN_CLAMPED, F110_RAY_FXN_PADDED,
       F110_RAY_FXS };
enum { F110_TABLE_TILED = 0, F110_TABLE_ROWMAJOR, F110_TABLE_PADDED };
typedef struct f110_ray_knobs {
    int32_t kernel;       /* f110_debug_ray_kernel: 1, 2 or 3, after f110_create's fallbacks */
    int32_t lanes;        /* rays per lane of the fixed-point kernels (1 or 2) */
    int32_t refill;       /* k_rays_fxs's waves per car (0: off) */
    int32_t fxs_lds;      /* k_rays_fxs in 8-wave blocks with the theta table in LDS (a shared device) */
    int32_t count_slots;  /* f110_debug_set_simt */
    int32_t wtrace;       /* a wave trace is armed for this launch */
    int32_t heavy_list;   /* the context has a heavy-first list, */
    int32_t heavy_on;     /*   keeps it up (the launch writes the per-wave costs), */
    int32_t heavy_use;    /*   and this launch runs it (steps, not resets); */
    int32_t heavy_cap;    /*   its capacity in waves */
    int32_t has_rm, has_rmp;  /* the clamped row-major / the padded EDT table exists */
    int32_t fxs_ok;       /* the padded table's rows and columns are below 2^20 */
    int32_t rotated;      /* the map's origin has a yaw */
    int32_t E, A, B, theta_dis, ray_wpb;
    int32_t has_geo;      /* the pair-geometry buffer exists (A >= 2) */
} f110_ray_knobs;
typedef struct f110_ray_plan {
    int32_t family;                                /* F110_RAY_* */
    int32_t rot, mask, handoff, lds, count, trace; /* the kernel's template flags */
    uint32_t grid, block;
    int32_t wpb, nch, G4, HB, geo_blocks;          /* RayArgs' launch shape */
    int32_t table;                                 /* F110_TABLE_*: the EDT the launch reads */
    int32_t wcost;                                 /* the launch writes the per-wave cost bytes */
    int32_t geo_ready;                             /* the launch computes the pair geometry */
} f110_ray_plan;
/* The plan of a launch with these knobs (masked: f110_reset with an env mask).  Host test hook. */
F110_API int f110_host_ray_plan(const f110_ray_knobs *in, int32_t masked, f110_ray_plan *out);
/* The size rules of f110_create (device_cars = own_cars, contexts = 1) and
 * f110_set_device_share: out = {rays per lane, k_rays_fxs's waves per car,
 * heavy-first on, fxs_lds} for a context of own_cars on a device that traces
 * device_cars at once in `contexts` contexts, whose ray kernel is `kernel` and
 * which may build the padded table (pad_allowed).  Host test hook. */
F110_API int f110_host_ray_rules(int64_t own_cars, int64_t device_cars, int32_t contexts, int32_t kernel,
                                 int32_t pad_allowed, int32_t out[4]);

/* ---- host-side test hooks (no device work) -------------------------------
 * The lookup tables f110_create uploads: ScanSimulator2D sines/cosines
 * (laser_models.py:379-381) and RaceCar's class-level beam tables
 * (base_classes.py:122-158).  Any pointer may be NULL. */
F110_API void f110_host_tables(int32_t theta_dis, int32_t n_beams, double fov, const f110_params *p,
                               double *sines, double *cosines, double *angles, double *beam_cos, double *side);
/* get_scan's sequentially accumulated beam index (laser_models.py:167-184)
 * for every beam at yaw, evaluated through the run decomposition the kernels
 * use.  Returns the number of runs (>0) or a negative error. */
F110_API int f110_host_beam_indices(double yaw, double fov, int32_t theta_dis, int32_t n_beams,
                                    double *theta_index_out);
/* 1 when k_agents' run builder (build_beam_runs_fast) gives the same runs as
 * build_beam_runs at yaw, 0 when not, < 0 on error (host). */
/* cr_sincos's branch-free common case (k_agents' dynamics): ok[i] = 1 where it applies, and
 * there sn / cs are cr_sincos's values (host). */
F110_API void f110_host_sincos_fast(const double *x, int64_t n, double *sn, double *cs, uint8_t *ok);
/* The kinematic model's (tan, cos) from one table evaluation: where ok_t the correctly rounded
 * tan, where ok_c cr_sincos's cos (host). */
F110_API void f110_host_tan_cos_fast(const double *x, int64_t n, double *t, double *c, uint8_t *ok_t, uint8_t *ok_c);
F110_API int f110_host_beam_runs_agree(double yaw, double fov, int32_t theta_dis, int32_t n_beams);

/* xy_2_rc's cell (laser_models.py:55-104) for n points xy [n][2] on an H x W
 * map, through the three device mappings: lin_out[n][3] = row-major index
 * with the IEEE divide (cell_index), with the guarded fast quotient
 * (cell_index_fast), and the 4x4-tiled mapping of the ray kernel translated
 * back to row-major.  Out-of-map points give H*W-1 (the reference's
 * dt[-1, -1]).  Host only; the CPU tests check the three agree on boundary
 * points. */
F110_API int f110_host_cell_index(int32_t H, int32_t W, double resolution, const double origin[3], const double *xy,
                                  int64_t n, int64_t *lin_out);

/* The EDT table f110_create uploads for the fixed-point ray kernels, built on
 * the host: kind 0 the row-major table (rows of W + 1 cells rounded up to 16,
 * dt[-1,-1] in the padding, a 0.0 zero cell after the last row), kind 1 the
 * table padded by `pad` cells of dt[-1,-1] on every side (rows of 511 mod 512
 * cells; not built past its 32-bit / 24-bit offset limits: returns 0).
 * Returns the length in doubles; fills out[] when out_len suffices; meta =
 * {rows, cols, zero-cell byte offset or -1}.  Host test hook. */
F110_API int64_t f110_host_map_table(const uint32_t *edt_k, int32_t H, int32_t W, double res, int32_t kind,
                                     int32_t pad, double *out, int64_t out_len, int64_t meta[3]);

/* The beam-index ranges (r0a..r0b, r1a..r1b; empty when a > b) the agent
 * ray_cast visits for an opponent box whose angular window at the scan
 * origin is center +- half (world frame), for a car at yaw.  Host only; the
 * CPU tests check they contain every beam inside the window. */
/* Host copy of the device's cr_sincos (the ray_cast / box / dynamics sin and
 * cos: double-double evaluation, one rounding, i.e. correctly rounded).  It
 * equals NumPy's (glibc's) np.sin / np.cos except where glibc is itself off
 * by one ulp (< 0.3 % of the sampled arguments, test_cr_sincos_matches_numpy);
 * on those the device differs from the reference's trig by that ulp, which
 * the non-exact budgets (tests/golden/nonexact_beams.json) pin.  Test hook,
 * no reference counterpart. */
F110_API void f110_host_sincos(const double *x, int64_t n, double *sn, double *cs);
/* The same with the table path off (every value by the double-double
 * series): f110_host_sincos must give the same bits (test hook). */
F110_API void f110_host_sincos_series(const double *x, int64_t n, double *sn, double *cs);
/* NumPy's float32 np.cos (cos_op != 0) / np.sin over n values, as the
 * device evaluates F110Env.reset's float32 start_rot (test hook). */
F110_API void f110_host_np_sincosf(const float *x, int64_t n, int32_t cos_op, float *out);
F110_API void f110_host_window_ranges(double yaw, double fov, int32_t n_beams, double center, double half,
                                      int32_t ranges_out[4]);

/* f110_set_param_randomization's validation of lo / hi [n_agents] against the
 * agents' params [n_agents], without a context: F110_OK, or F110_E_INVALID with
 * the field named in f110_last_error (non-finite, lo > hi, width / length /
 * lidar_max not the agent's).  Host test hook. */
F110_API int f110_host_check_param_ranges(const f110_params *lo, const f110_params *hi,
                                          const f110_params *agent_params, int32_t n_agents);
/* The row a resetting car draws (the device's param_draw on the host): car
 * `agent` of global env `env` in episode `episode` under (lo, hi, seed); out's
 * width / length / lidar_max are lo's.  Host test hook. */
F110_API int f110_host_param_draw(uint64_t seed, int64_t env, int32_t agent, uint64_t episode, const f110_params *lo,
                                  const f110_params *hi, f110_params *out);

/* f110_set_spawn_randomization's validation of ranges [n_agents] without a
 * context (n_spawn: the rows of the context's spawn table, 0 = none): F110_OK,
 * or F110_E_INVALID with the field named in f110_last_error.  Host test hook. */
F110_API int f110_host_check_spawn_ranges(const f110_spawn_range *ranges, int32_t n_agents, int32_t n_spawn);
/* The start states n resetting envs draw (the device's row rule,
 * csrc/f110_spawn.h, on the host): out [n][n_agents][4] = (x, y, yaw, speed)
 * of every car of env envs[i] in episode episodes[i] (NULL: 0) under (ranges,
 * seed), over the HOST EDT edt [H*W] in metres (row-major, the MapView layout)
 * with the map's resolution and origin.
 * poses != NULL: f110_reset -- the base poses are poses [n][n_agents][3] and
 * the gap does not apply.  poses == NULL: an autoreset from spawn
 * [n_spawn][n_agents][3] -- the env's row k is rows[i] when rows != NULL, else
 * the context's draw under ctx_seed for the finished episode episodes[i] - 1.
 * reset_f32: the poses rounded as under F110_F32 resets.  rows_out
 * [n][n_agents] (or NULL): the table row each car's base pose came from (-1
 * with poses).  Same validation as f110_set_spawn_randomization.  Host test
 * hook: the CPU suite and the GPU tests share one statement of the semantics. */
F110_API int f110_host_spawn_rows(const f110_spawn_range *ranges, int32_t n_agents, uint64_t seed, uint64_t ctx_seed,
                                  const double *edt, int32_t H, int32_t W, double resolution, const double origin[3],
                                  const double *spawn, int32_t n_spawn, const double *poses, const int32_t *rows,
                                  const int64_t *envs, const uint64_t *episodes, int64_t n, int32_t reset_f32,
                                  double *out, int32_t *rows_out);

/* f110_set_episode_limits' validation without a context: F110_OK, or
 * F110_E_INVALID with the argument named in f110_last_error (negative
 * max_steps / stall_steps, negative or non-finite stall_speed).  Host test hook. */
F110_API int f110_host_check_episode_limits(int64_t max_steps, double stall_speed, int32_t stall_steps);
/* f110_episode_stats over HOST arrays (same arguments, no scratch, no stream):
 * the device's per-env update and totals merge, run in ascending env order.
 * The device differs only in the order return_sum is added up (f110.h).  Host
 * test hook: the CPU suite and the GPU tests share one statement of the
 * semantics. */
F110_API int f110_host_episode_stats(const double *rewards, const uint8_t *terminated, const uint8_t *truncated,
                                     const uint8_t *was_reset, int64_t n_envs, f110_episode_state *state,
                                     double *last_return, int32_t *last_length, uint8_t *finished,
                                     f110_episode_totals *totals);

/* f110_ddpg_actor_explore_env's per-row epilogue over HOST arrays: the same function the kernel runs
 * (explore_one, csrc/f110_head_rows.h), on given actions act [n_rows][nout] f32 (f110_ddpg_actor_head's
 * act) and given draws normals [n_rows][nout] f32.  ou_x, reset, eval_mask, kind, theta / mu / dt,
 * low / high, the {sigma, call index} pair state_in and decay / sigma_min as there; writes out
 * [n_rows][nout] (packed), updates ou_x and, when state_out is not NULL, writes the decayed pair.
 * Same validation (F110_E_INVALID).  Host test hook: the CPU suite and the GPU tests share one
 * statement of the semantics. */
F110_API int f110_host_explore_rows(const float *act, const float *normals, int64_t n_rows, int32_t nout,
                                    int32_t kind, double *ou_x, double theta, double mu, double dt,
                                    const uint8_t *reset, const uint8_t *eval_mask, const double *state_in,
                                    double *state_out, double decay, double sigma_min, const float *low,
                                    const float *high, float *out);

/* The TD3 heads' row rules over HOST arrays: the same functions the kernels run (td3_smooth_one,
 * td3_row, csrc/f110_head_rows.h).  f110_host_td3_smooth_rows: f110_td3_target_action's epilogue on
 * given actions act and draws normals ([n_rows][nout] f32), scale / low / high [nout]; writes out
 * [n_rows][nout].  f110_host_td3_rows: f110_td3_critic_step's row rule on given head outputs q1t,
 * q2t, q1, q2 and r, d, w ([B] f32), g the loss gradient (a host scalar; gb = g / B); writes td1,
 * td2, dq1, dq2, prio (the kernel's td) and wl (the row's loss term), each [B].  Same validation
 * (F110_E_INVALID).  Host test hooks: the CPU suite and the GPU tests share one statement of the
 * semantics. */
F110_API int f110_host_td3_smooth_rows(const float *act, const float *normals, int64_t n_rows, int32_t nout,
                                       float policy_noise, float noise_clip, const float *scale, const float *low,
                                       const float *high, float *out);
F110_API int f110_host_td3_rows(const float *r, const float *d, float gamma, const float *q1t, const float *q2t,
                                const float *q1, const float *q2, const float *w, float g, int64_t B, float *td1,
                                float *td2, float *dq1, float *dq2, float *prio, float *wl);

/* One f110_nstep_push over HOST arrays: the same per-env function the kernel runs (nstep_update,
 * csrc/f110_learner_args.h), envs in ascending order.  len / head [n_envs], ret / k [n_envs][n_step],
 * win_obs [n_envs][n_step][obs_dim] and win_act [n_envs][n_step][act_dim] are the windows
 * (f110_nstep_arrays' layout; zero = fresh), updated in place; obs / act / next_obs are packed
 * rows.  Writes the emitted rows, in the order the device appends them, to out_obs / out_next_obs
 * [.][obs_dim], out_act [.][act_dim], out_reward / out_done [.] (room for n_envs * n_step rows)
 * and their number to out_count.  Same validation (F110_E_INVALID); capacity > 0 also checks
 * n_envs * n_step <= capacity as a push into such a ring would.  Host test hook: the CPU suite
 * and the GPU tests share one statement of the semantics. */
F110_API int f110_host_nstep(int64_t n_envs, int32_t n_step, double gamma, int32_t obs_dim, int32_t act_dim,
                             int64_t capacity, int32_t *len, int32_t *head, double *ret, int32_t *k, float *win_obs,
                             float *win_act, const float *obs, const float *act, const double *reward,
                             const float *next_obs, const uint8_t *terminated, const uint8_t *truncated,
                             const uint8_t *was_reset, float *out_obs, float *out_act, float *out_reward,
                             float *out_next_obs, float *out_done, int64_t *out_count);

/* f110_repeat_hold and f110_repeat_push over HOST arrays: the same per-env function the kernel runs
 * (repeat_update, csrc/f110_repeat.h), envs in ascending order.  k / ret [n_envs], s_obs
 * [n_envs][obs_dim] and s_act [n_envs][act_dim] are the handle's state (f110_repeat_arrays' layout;
 * zero = fresh), updated in place; obs / act / next_obs are packed rows.  The hold rewrites act in
 * place and writes decision [n_envs] (may be NULL).  The push writes the emitted rows, in the order
 * the device appends them, to out_obs / out_next_obs [.][obs_dim], out_act [.][act_dim], out_reward
 * / out_done [.] (room for n_envs rows) and their number to out_count.  Same validation
 * (F110_E_INVALID); capacity > 0 also checks n_envs <= capacity as a push into such a ring would.
 * Host test hooks: the CPU suite and the GPU tests share one statement of the semantics. */
F110_API int f110_host_repeat_hold(int64_t n_envs, int32_t obs_dim, int32_t act_dim, const int32_t *k, float *s_obs,
                                   float *s_act, const float *obs, float *act, uint8_t *decision);
F110_API int f110_host_repeat_push(int64_t n_envs, int32_t repeat, double gamma, int32_t obs_dim, int32_t act_dim,
                                   int64_t capacity, int32_t *k, double *ret, const float *s_obs, const float *s_act,
                                   const double *reward, const float *next_obs, const uint8_t *terminated,
                                   const uint8_t *truncated, const uint8_t *was_reset, float *out_obs, float *out_act,
                                   float *out_reward, float *out_next_obs, float *out_done, int64_t *out_count);

/* f110_agent_obs over HOST arrays (same arguments, no stream): the same scan entry the kernels run
 * (obs_scan_value, csrc/f110_env_rows.h) and the same pose-group order.  Same validation
 * (F110_E_INVALID).  Host test hook: the CPU suite and the GPU tests share one statement of the
 * semantics. */
F110_API int f110_host_agent_obs(const float *scans, int64_t scan_env_stride, const float *obs, int64_t obs_stride,
                                 int64_t n_envs, int32_t n_agents, int32_t n_beams, int32_t agent, float lidar_max,
                                 float *out, int64_t out_stride);

/* f110_pure_pursuit over HOST arrays (same arguments, no stream): the 5 nearest midpoints by a full
 * scan (ties: lower index), then the device's f64 operations in the device's order, the same
 * cr_sincos and the same row rule (csrc/f110_pursuit.h); atan is the host libm's.  Needs only the
 * track's host arrays, so a track built with device < 0 will do.  Same validation
 * (F110_E_INVALID).  Host test hook: the CPU suite and the GPU tests share one statement of the
 * semantics. */
F110_API int f110_host_pure_pursuit(const f110_track *track, const f110_pursuit_params *params, const float *poses,
                                    int64_t n_rows, int64_t pose_stride, const double *row_speed,
                                    const uint8_t *row_mask, float *actions, int64_t action_stride, double *aux);

/* f110_race_stats over HOST arrays (same arguments, no scratch, no stream): the projection of
 * f110_host_pure_pursuit, the same row rule and totals merge (csrc/f110_race.h), envs in ascending
 * order.  The device differs only in the order progress_sum and lead_sum are added up (f110.h).
 * Needs only the track's host arrays, so a track built with device < 0 will do.  Same validation
 * (F110_E_INVALID) otherwise.  Host test hook: the CPU suite and the GPU tests share one statement
 * of the semantics. */
F110_API int f110_host_race_stats(const f110_track *track, const f110_race_params *params, const float *ego,
                                  const float *opp, int64_t stride, const uint8_t *terminated,
                                  const uint8_t *truncated, const uint8_t *was_reset, int64_t n_envs,
                                  f110_race_state *state, double *cur, double *last_progress, double *last_lead,
                                  int32_t *last_length, uint8_t *result, f110_race_totals *totals);

/* f110_track_obs over HOST arrays (same arguments, no stream): the projection of
 * f110_host_pure_pursuit (with the segment it came from), then the same row rule
 * (csrc/f110_track_obs.h) -- no libm call but sqrt, so the device's bits.  Needs only the track's
 * host arrays, so a track built with device < 0 will do.  Same validation (F110_E_INVALID)
 * otherwise.  Host test hook: the CPU suite and the GPU tests share one statement of the semantics. */
F110_API int f110_host_track_obs(const f110_track *track, const f110_track_obs_params *params, const double *state,
                                 int64_t n_envs, int32_t n_agents, int32_t seat, int32_t other, float *out,
                                 int64_t out_stride);

/* f110_scan_obs_push over HOST arrays: the same row rule (csrc/f110_scan_obs.h), envs in ascending
 * order, with the shape and the state passed in: ring [n_envs][D][K] float32 and head [n_envs] int32
 * (f110_scan_obs_arrays' layout; head -1 = empty), updated in place.  Same validation
 * (F110_E_INVALID), and a head outside [-1, D) is refused too.  Pure host code: the sanitizer
 * program links it.  Host test hook: the CPU suite and the GPU tests share one statement of the
 * semantics. */
F110_API int f110_host_scan_obs_push(const f110_scan_obs_params *params, int64_t n_envs, int32_t n_beams,
                                     int32_t n_mid, int32_t n_tail, const float *rows, int64_t row_stride,
                                     const uint8_t *reset, float *ring, int32_t *head, float *out,
                                     int64_t out_stride);

/* What f110_sensor_create refuses of the ranges, without a device (F110_E_INVALID with the reason). */
F110_API int f110_host_check_sensor_params(const f110_sensor_params *params, int32_t n_beams);

/* f110_sensor_apply over HOST arrays: the same row rule (csrc/f110_sensor.h), envs in ascending
 * order, with the shape, the seed, the mask (host u8 or NULL) and the state passed in: param_rows
 * [n_envs][10] float32, episode and step [n_envs] int32 (f110_sensor_arrays' layout; episode -1 = no
 * apply yet), updated in place.  Same validation (F110_E_INVALID) as create and apply, and an
 * episode below -1 is refused too.  Pure host code: the sanitizer program links it.  Host test hook:
 * the CPU suite and the GPU tests share one statement of the semantics. */
F110_API int f110_host_sensor_apply(const f110_sensor_params *params, int64_t n_envs, int32_t n_beams,
                                    int32_t n_mid, int32_t n_tail, float range_max, uint64_t seed,
                                    int64_t env_offset, const uint8_t *env_mask, const float *rows,
                                    int64_t row_stride, const uint8_t *reset, float *param_rows, int32_t *episode,
                                    int32_t *step, float *out, int64_t out_stride);

#ifdef __cplusplus
}
#endif
#endif /* F110_DEBUG_H */
