/*
 * f110.h — C ABI of libf110.so, the MI355X (gfx950) batched F1TENTH step.
 *
 * This is the drop-in boundary for the per-step hot path of f110_gym
 * (ahoop004/f110_gymnasium_ros2_jazzy, paths below are relative to
 * f110_gymnasium/gym/f110_gym/envs/).  The reference has no FFI: its hot path
 * is a set of Numba @njit functions driven by the Python classes RaceCar /
 * Simulator / F110Env.  Each entry point below names the reference interface
 * it replaces.  INTEGRATION.md shows the ctypes binding the reference side
 * would add.
 *
 * Conventions
 *  - Plain C types only.  Every array argument of f110_reset / f110_step /
 *    f110_*_batch is a DEVICE pointer owned by the caller (e.g. a
 *    torch.Tensor's data_ptr()).  f110_edt_k and f110_create take HOST
 *    pointers (cold path, once per map).
 *  - Work is enqueued asynchronously on the hipStream_t passed as `stream`
 *    (NULL = the default stream).  No call below synchronises the device or
 *    allocates memory after f110_create.
 *  - Return value: 0 on success, a negative F110_E* code on error;
 *    f110_last_error() describes the last error of the calling thread.
 *  - One context = one device, one map, one batch of n_envs x n_agents cars.
 *    A context is not thread-safe; use one per host thread.  (The reference
 *    shares a class-level ScanSimulator2D across every env in the process,
 *    base_classes.py:64-67,118-120; contexts share nothing.)
 *  - Layouts: agent index g = env * n_agents + agent.  State is kept on the
 *    device as structure-of-arrays fp64: state[k * n_envs*n_agents + g],
 *    k = 0..6 = [x, y, steer, v, yaw, yaw_rate, slip] (base_classes.py:97).
 */
#ifndef F110_H
#define F110_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define F110_API __attribute__((visibility("default")))
#else
#define F110_API
#endif

#define F110_ABI_VERSION 3  /* 2: f110_outputs.obs_stride; 3: f110_adam_step target / tau, head dh_mask,
                                 f110_debug_* names (include/f110_debug.h), f110_set_device_share */

#define F110_OK 0
#define F110_E_INVALID (-1)  /* bad argument / shape */
#define F110_E_HIP (-2)      /* HIP runtime error */
#define F110_E_NOMAP (-3)    /* ScanSimulator2D.scan without a map (laser_models.py:445-446) */
#define F110_E_NODEVICE (-4) /* no gfx950 device */
#define F110_E_ALLOC (-5)

#define F110_F32 0  /* action dtypes for f110_step */
#define F110_F64 1

#define F110_INTEGRATOR_RK4 1   /* base_classes.py:40-42 */
#define F110_INTEGRATOR_EULER 2

/* Vehicle parameters: F110Env default params dict (f110_env.py:132-156). */
typedef struct f110_params {
    double mu, C_Sf, C_Sr, lf, lr, h, m, I;
    double s_min, s_max, sv_min, sv_max, v_switch, a_max, v_min, v_max;
    double width, length, lidar_max;
} f110_params;

/* Simulator / sensor configuration (F110Env.__init__ kwargs f110_env.py:104-186,
 * RaceCar.__init__ base_classes.py:69-115, ScanSimulator2D.__init__
 * laser_models.py:360-381). */
typedef struct f110_config {
    int32_t n_envs;      /* environments in this context (this rank's shard) */
    int32_t n_agents;    /* cars per environment, 1..8 */
    int32_t n_beams;     /* 1080 */
    int32_t theta_dis;   /* 2000 */
    int32_t integrator;  /* F110_INTEGRATOR_RK4 (F110Env default) */
    int32_t ego_idx;     /* 0 */
    int32_t autoreset;   /* 1: a terminated env is reset (spawn table) at its next f110_step */
    int32_t _pad;
    double fov;          /* 4.7 */
    double eps;          /* 1e-4 */
    double max_range;    /* 30.0 */
    double time_step;    /* 0.01 */
    double lidar_dist;   /* 0.0 */
    double ttc_thresh;   /* 0.005 (base_classes.py:115) */
    double noise_std;    /* 0.01 (laser_models.py:429); 0 disables scan noise */
    int64_t env_offset;  /* global id of env 0 of this context (RNG keying across ranks) */
    uint64_t seed;       /* scan-noise / autoreset seed (F110Env 'seed' kwarg) */
} f110_config;

/* Per-step outputs (all optional except where noted; NULL = not written). */
typedef struct f110_outputs {
    float *obs;          /* [n_envs][n_beams + 4*n_agents]: F110Env._pack_flat_obs
                            (f110_env.py:552-584) generalised to A agents; A=2 -> 1088 */
    float *scans;        /* [n_envs][n_agents][n_beams] f32 ranges (info["scans"], :599) */
    double *scans_f64;   /* [n_envs][n_agents][n_beams] fp64 ranges (Simulator.step obs['scans']) */
    uint8_t *collisions; /* [n_envs][n_agents] 0/1 (Simulator.collisions) */
    uint8_t *terminated; /* [n_envs] F110Env._check_done (f110_env.py:310-352) */
    uint8_t *was_reset;  /* [n_envs] 1 where this call reset the env (autoreset / f110_reset) */
    float *lap_times;    /* [n_envs][n_agents] */
    float *lap_counts;   /* [n_envs][n_agents] */
    double *sim_time;    /* [n_envs] F110Env.current_time */
    int64_t obs_stride;  /* floats from one obs row to the next (>= n_beams + 4*n_agents); 0 = packed.
                            A 128-B multiple (1088 for A = 1) keeps every 64-beam chunk of a row on
                            whole cache lines: the ray kernel's obs stores are not split. */
} f110_outputs;

typedef struct f110_ctx f110_ctx;

/* ---- library ---------------------------------------------------------- */
F110_API int f110_abi_version(void);
F110_API const char *f110_last_error(void);
/* Fills the F110Env defaults (f110_env.py:132-156, :159-186). */
F110_API void f110_default_params(f110_params *p);
F110_API void f110_default_config(f110_config *c);

/* ---- map (cold path, host memory) -------------------------------------- */
/* Exact squared EDT of an occupancy grid: k[r*W+c] = squared distance (in
 * cells) from (r,c) to the nearest occupied cell (free_mask == 0).
 * Replaces get_dt / scipy.ndimage.distance_transform_edt
 * (laser_models.py:40-53, :425): dt = resolution * sqrt((double)k), bit-for-bit.
 * free_mask is the image after ScanSimulator2D.set_map's flip + threshold
 * (laser_models.py:397-404). */
F110_API int f110_edt_k(const uint8_t *free_mask, int32_t H, int32_t W, uint32_t *k_out);

/* ---- context ------------------------------------------------------------
 * Replaces Simulator.__init__ + set_map (base_classes.py:478-524) and
 * ScanSimulator2D.__init__/set_map (laser_models.py:360-427).  edt_k: HOST
 * [H*W] from f110_edt_k.  origin = map yaml 'origin' (x, y, yaw).
 * spawn_poses: optional HOST [n_spawn][n_agents][3] table used by autoreset. */
F110_API int f110_create(f110_ctx **out, int32_t device, const f110_config *cfg, const f110_params *params,
                const uint32_t *edt_k, int32_t H, int32_t W, double resolution, const double origin[3],
                const double *spawn_poses, int32_t n_spawn);
F110_API int f110_destroy(f110_ctx *ctx);

/* ---- per step (device pointers, async on stream) ----------------------- */
/* Replaces F110Env.reset (f110_env.py:425-472) = Simulator.reset
 * (base_classes.py:627-643) + RaceCar.reset (:183-204) + the zero-action
 * step the reference performs inside reset (f110_env.py:457-458).
 * poses: [n_envs][n_agents][3] f64.  env_mask: [n_envs] u8, NULL = all envs.
 * Only masked envs are touched; their outputs are written. */
F110_API int f110_reset(f110_ctx *ctx, const double *poses, const uint8_t *env_mask, const f110_outputs *out,
               void *stream);

/* Replaces F110Env.step (f110_env.py:371-421) = Simulator.step
 * (base_classes.py:566-625): per agent update_pose (steer delay, pid, RK4 of
 * vehicle_dynamics_st, clamps) + ScanSimulator2D.scan (+ noise), GJK
 * collision_multiple, TTC (check_ttc_jit), agent ray_cast, obs packing,
 * _check_done.  actions: [n_envs][n_agents][2] (steer, velocity), f32
 * (F110Env's action_space dtype, f110_env.py:238-242) or f64 (Simulator.step
 * takes whatever control_inputs dtype it is given): actions_dtype = F110_F32 /
 * F110_F64. */
F110_API int f110_step(f110_ctx *ctx, const void *actions, int32_t actions_dtype, const f110_outputs *out,
                       void *stream);
/* n_steps consecutive f110_step calls with resident actions: step t reads the
 * [n_envs][n_agents][2] block at actions + t * step_stride elements
 * (step_stride 0 = packed, n_envs * n_agents * 2) -- a rollout of open-loop
 * actions; every output holds the last step's values, exactly as after the n
 * calls (the three-launch step runs n times, no host work in between). */
F110_API int f110_step_n(f110_ctx *ctx, const void *actions, int32_t actions_dtype, int32_t n_steps,
                         int64_t step_stride, const f110_outputs *out, void *stream);

/* Replaces F110Env.update_params / Simulator.update_params
 * (f110_env.py:487-498, base_classes.py:527-546): agent_idx < 0 updates every
 * car, otherwise one car (out of range -> F110_E_INVALID, the reference's
 * IndexError).  Like RaceCar.params, the update reaches the car's dynamics
 * (update_pose) and the opponent boxes of its agent ray_cast
 * (base_classes.py:223); the GJK boxes (Simulator.params, :562), the TTC
 * side distances (class-level, :122-158) and the obs lidar_max keep the
 * params given to f110_create, as in the reference.  params is a host
 * pointer; the call is ordered on `stream` and returns when it is applied. */
F110_API int f110_set_params(f110_ctx *ctx, const f110_params *params, int32_t agent_idx, void *stream);

/* ---- per-env vehicle params (no reference counterpart: the reference has one
 * params dict per car) ------------------------------------------------------
 * The 16 dynamics fields (mu .. v_max, the leading doubles of f110_params) may
 * differ from env to env: the context then keeps a device table of them per
 * car, which the cars' update_pose (pid, clips, RK4 / Euler, clamps) reads
 * instead of the per-agent params.  width, length and lidar_max do NOT vary
 * per env: the car boxes (agent ray_cast, GJK), the TTC side distances and the
 * obs scale keep reading the per-agent / f110_create params, and a row whose
 * width, length or lidar_max differs from its agent's current f110_set_params
 * value is refused.
 * Precedence: with a table set, the table's dynamics win.  f110_set_params
 * still updates the per-agent params (the boxes, and the dynamics the context
 * returns to when the table is dropped) and does not touch the table.
 *
 * f110_set_env_params: params is a HOST array [n_envs][n_agents]; NULL drops
 * the table (and the randomization with it): back to the per-agent params.
 * F110_E_INVALID, with the field named in f110_last_error, for a non-finite
 * value or a differing width / length / lidar_max; the table is then
 * unchanged.  Ordered on `stream`, applied when the call returns. */
F110_API int f110_set_env_params(f110_ctx *ctx, const f110_params *params, void *stream);
/* The params in force, out = HOST [n_envs][n_agents]: the table's rows if one
 * is set (under randomization, the cars drawn at each env's last reset), else
 * the per-agent params for every env.  Waits for `stream`. */
F110_API int f110_get_env_params(f110_ctx *ctx, f110_params *out, void *stream);
/* Domain randomization on the device: from now on a car that resets -- in
 * f110_reset (its masked envs) or by autoreset inside f110_step / f110_step_n,
 * a captured graph included -- redraws its 16 dynamics fields before the
 * reset's own zero-action step, field = lo + u * (hi - lo) with u = r * 2^-32
 * in [0, 1) for a 32-bit Philox4x32-10 draw r (hi == lo gives exactly lo), and
 * stores the row in the table; cars that do not reset keep theirs.  The draw
 * is keyed by (seed, global env id = env_offset + env, agent, field, episode):
 * episode is 0 for f110_reset and counts the env's autoresets since, so an
 * explicit reset reproduces the same cars whatever ran before it, and a shard
 * of the envs (env_offset) draws what the whole batch draws for them.
 * lo, hi: HOST [n_agents]; NULL, NULL turns it off and keeps the table as it
 * stands.  Allocates the table if there is none, filled with the per-agent
 * params.  F110_E_INVALID (field named in f110_last_error, checked before any
 * device call) for a non-finite value, lo > hi, or a width / length /
 * lidar_max of lo or hi that differs from the agent's.  Ordered on `stream`,
 * applied when the call returns. */
F110_API int f110_set_param_randomization(f110_ctx *ctx, const f110_params *lo, const f110_params *hi, uint64_t seed,
                                          void *stream);

/* ---- spawn randomization (no reference counterpart: the reference resets to
 * the poses its caller passes) ------------------------------------------------
 * The start state of an episode, drawn on the device where the reset happens:
 * a lateral offset from the base pose, a heading offset, a start speed and,
 * for autoresets, the distance to the ego's spawn row along the table.  One
 * range block per agent: */
typedef struct {
    double  lateral[2];   /* m, along the left normal of the table heading            */
    double  heading[2];   /* rad, added to the table yaw                              */
    double  speed[2];     /* m/s, the car's state[3] before the reset's own step      */
    int32_t gap[2];       /* table rows, 0 <= lo <= hi; {0,0}: the agent's own column */
    double  behind;       /* in [0,1]: probability that the gap is counted backwards  */
    double  clearance;    /* m, >= 0: least EDT value accepted at the offset position */
} f110_spawn_range;
/* From now on a car that resets -- in f110_reset (its masked envs) or by
 * autoreset inside f110_step / f110_step_n, a captured graph included -- starts
 * from a drawn state instead of the base pose at rest.
 * Draw: Philox4x32-10 under f110_set_param_randomization's key (seed, global
 * env id = env_offset + env), counter (episode lo, episode hi, tag 0x5FA17,
 * agent * 2 + j): block j = 0 gives, word by word, the gap magnitude, the
 * behind decision, the lateral offset and the heading offset; word 0 of block
 * j = 1 the speed.  A real value is lo + u * (hi - lo) with u = r * 2^-32 in
 * [0, 1) (hi == lo gives exactly lo), the gap magnitude lo + r % (hi - lo + 1),
 * and the gap counts backwards when u < behind.  episode is 0 for f110_reset
 * and the finished episode's number + 1 for an autoreset, as for the param
 * draw: an explicit reset reproduces the same starts whatever ran before it,
 * and a shard of the envs (env_offset) draws what the whole batch draws for
 * them.
 * Base pose: in f110_reset the caller's pose; the gap does not apply there.
 * In an autoreset, with k the env's spawn row as without the feature, an agent
 * whose gap is {0,0} takes column `agent` of row k, any other agent column 0
 * of row (k + mag) mod n_spawn, or (k - mag) mod n_spawn when the gap counts
 * backwards: the table must then be ordered along the track (the bundled
 * centerline tables are).
 * Offset: with (sin, cos) of the base yaw th, x = px + d * (-sin), y = py +
 * d * cos, yaw = th + dth.  Clearance: d, d/2, d/4, d/8 are tried in that
 * order and the first whose position reads an EDT value >= clearance is
 * taken (a position outside the map reads the map's last cell, as every
 * lookup does); when none does, d = 0, which is always accepted.  Heading and
 * speed are never adjusted.  Under F110_F32 resets x, y and yaw are rounded to
 * float32 after the perturbation (start_rot and the lap logic see the rounded,
 * perturbed pose); the speed stays float64.
 * Precedence inside a reset: the pose draw, then the param draw
 * (f110_set_param_randomization), then the reset's own zero-action step, which
 * starts from (x, y, yaw, speed) with every other state entry 0.
 * The ranges of two agents are not checked against each other: cars drawn
 * onto one another collide in the reset's own step, the episode ends there and
 * the next one draws afresh.
 * ranges: HOST [n_agents]; NULL turns it off (resets are the base poses at
 * rest again).  F110_E_INVALID, with the field named in f110_last_error and
 * before any device call, for a non-finite value, lo > hi, a negative gap,
 * behind outside [0, 1], a negative clearance, or a non-zero gap on a context
 * created without a spawn table.  Ordered on `stream`, applied when the call
 * returns. */
F110_API int f110_set_spawn_randomization(f110_ctx *ctx, const f110_spawn_range *ranges, uint64_t seed, void *stream);
/* What each car's last reset under spawn randomization put into its state
 * before the reset's own zero-action step: out = device [4][n_envs*n_agents]
 * f64 (x, y, yaw, speed; SoA like f110_get_state).  Rows of cars that have not
 * reset since the feature came on are 0; resets while it is off leave the rows
 * as they stand.  F110_E_INVALID on a context that never turned it on.  Async
 * on `stream`. */
F110_API int f110_get_spawn_state(f110_ctx *ctx, double *out, void *stream);

/* ---- episode limits (no reference counterpart: the reference steps one env
 * from a Python loop that simply stops; gymnasium's TimeLimit wrapper is a host
 * wrapper, and here the reset happens on the device) --------------------------
 * Truncation in the step's epilogue.  Per env, n = steps since the env's last
 * reset (0 after the reset's own zero-action step, +1 in every step that does
 * not reset the env) and s = the stall counter: after a non-reset step, with v
 * the ego's state[3] after the TTC response, s = |v| < stall_speed ? s + 1 : 0;
 * 0 after a reset.  An env that did not terminate in the step gets
 *   truncated = (max_steps && n >= max_steps) ? 1          (time limit)
 *             : (stall_steps && s >= stall_steps) ? 2      (stall)
 *             : 0
 * so termination wins over truncation and the time limit over the stall; a
 * reset step (f110_reset, or an autoreset) writes 0.  With cfg.autoreset a
 * truncated env is reset at its next step exactly as a terminated one is (same
 * spawn draw, same param draw, same episode count, was_reset set); without it
 * the flag stays up while its condition holds and nothing else changes.  A
 * masked f110_reset zeroes n and s of the masked envs only.
 * max_steps 0 = no time limit, stall_steps 0 = no stall limit; with both 0 the
 * context is back on the limit-free path and `truncated` is dropped, never
 * written.  truncated: device [n_envs] u8 that every following f110_step /
 * f110_step_n / f110_reset writes (a masked reset: the masked envs), or NULL
 * (the limits still end episodes).  Turning the stall limit on (stall_steps
 * from 0) starts every env's s at 0.  F110_E_INVALID, with the argument named in
 * f110_last_error and before any device call, for a negative max_steps or
 * stall_steps or a negative / non-finite stall_speed.  Ordered on `stream`,
 * applied when the call returns. */
F110_API int f110_set_episode_limits(f110_ctx *ctx, int64_t max_steps, double stall_speed, int32_t stall_steps,
                                     uint8_t *truncated, void *stream);

/* Scan-noise source of the following f110_step / f110_reset calls.
 * noise: device [n_envs][n_beams] f64, or NULL for the built-in stream.
 * The reference draws the noise as rng.normal(0, std_dev, num_beams) from a
 * numpy Generator that every car re-creates with the same seed at reset
 * (laser_models.py:450-452, base_classes.py:119,204), so the agents of one
 * env see the same vector.  With a buffer set, each ray adds
 * noise[env][beam] to its clamped range instead of the device Philox draw
 * (noise_std is then unused).  The caller refills the buffer before each
 * call, ordered on the same stream; it must outlive the calls that read it.
 * The F110Env facade uses it to replay the reference's generator exactly. */
F110_API int f110_set_scan_noise(f110_ctx *ctx, const double *noise);

/* ---- state access ------------------------------------------------------- */
/* state: device [7][n_envs*n_agents] f64 (SoA, see header comment).
 * steer_buf: device [2][n_envs*n_agents] f64 ([newest, older]); steer_cnt:
 * device [n_envs*n_agents] i32 — RaceCar.steer_buffer (base_classes.py:108-109). */
F110_API int f110_get_state(f110_ctx *ctx, double *state, double *steer_buf, int32_t *steer_cnt, void *stream);
/* F110Env's lap bookkeeping as the device holds it (f110_env.py:310-352,
 * 441-451): start_rot[2][E] = cos(-th), sin(-th) of each env's ego reset
 * yaw (float64, or float32 values under F110_F32 resets) and toggles[E*A]
 * (toggle_list).  Device pointers (either may be NULL), async on `stream`. */
F110_API int f110_get_lap_state(f110_ctx *ctx, double *start_rot, int32_t *toggles, void *stream);
F110_API int f110_set_state(f110_ctx *ctx, const double *state, const double *steer_buf, const int32_t *steer_cnt,
                   void *stream);

/* ---- building blocks (device pointers) ----------------------------------
 * Replaces ScanSimulator2D.scan with rng=None (laser_models.py:429-454) =
 * get_scan/trace_ray (:106-186): poses [M][3] (x, y, yaw) -> scans [M][n_beams]
 * f64.  lookups [M][n_beams] i32 and hit_rc [M][n_beams][2] i32 (last EDT cell
 * read by each ray) are optional probes. */
F110_API int f110_scan_batch(f110_ctx *ctx, const double *poses, int64_t M, double *scans, int32_t *lookups,
                    int32_t *hit_rc, void *stream);

/* Replaces vehicle_dynamics_st (dynamic_models.py:123-176) on M states:
 * x [M][7], u [M][2] (steer velocity, acceleration) -> f [M][7]. */
F110_API int f110_dynamics_batch(f110_ctx *ctx, const double *x, const double *u, double *f, int64_t M, void *stream);

/* vehicle_dynamics_ks (dynamic_models.py:90-121) for M kinematic states:
 * x[M][5] = (x, y, steer, v, yaw), u[M][2] = (steer velocity, accel) ->
 * f[M][5], under the context's params (the KS model of the reference's
 * DynamicsTest KATs; the ST model's |v| < 0.5 branch uses the same terms).
 * Device pointers, async on `stream`.  Replaces: a loop of
 * vehicle_dynamics_ks calls. */
F110_API int f110_dynamics_ks_batch(f110_ctx *ctx, const double *x, const double *u, double *f, int64_t M,
                                    void *stream);

/* ---- collision building blocks (no context) --------------------------------
 * f110_collision_batch: collision(vertices1, vertices2) (collision_models.py:
 * 113-182, 2-D GJK, <= 1000 iterations) for M pairs: v1[M][4][2], v2[M][4][2]
 * -> out[M] (1 = overlap).  Replaces: a Python loop over collision().
 * f110_collision_multiple: collision_multiple(vertices) (collision_models.py:
 * 184-212) for M independent sets of N bodies: verts[M][N][4][2] ->
 * collisions[M][N] (0./1.) and idx[M][N] (partner index, -1. if none; the
 * last colliding pair in the reference's i < j loop order wins), 1 <= N <= 64.
 * Device pointers, async on `stream`. */
F110_API int f110_collision_batch(const double *v1, const double *v2, int64_t M, uint8_t *out, void *stream);
F110_API int f110_collision_multiple(const double *verts, int64_t M, int32_t N, double *collisions, double *idx,
                                     void *stream);

/* The dtype of the reset poses whose F110Env.reset semantics the following
 * resets follow (f110_env.py:441-451): F110_F32 (train_ddpg passes float32
 * options) rounds the reset / autoreset poses to float32 and evaluates the lap
 * logic's start_rot as NumPy's float32 cos / sin of the float32 yaw;
 * F110_F64 (the default) keeps float64.  Replaces: the dtype the consumer's
 * `options` array carries into F110Env.reset. */
F110_API int f110_set_reset_dtype(f110_ctx *ctx, int32_t dtype);

/* Scheduling hint for a caller that steps several contexts concurrently on one
 * device (e.g. sub-shards of one GPU's envs on separate streams): this context
 * is one of `contexts` whose ray passes run together, tracing `device_cars`
 * cars (envs x agents) in all.  The library then picks the ray kernel for the
 * device's load instead of this context's alone (DESIGN.md §3.3-3.4, §3.14,
 * §5.1: k_rays_fxs with 1 / 2 / 3 waves per car by the device's cars; with
 * other contexts, no heavy-first dispatch and, for single-agent contexts,
 * the 8-wave blocks that keep the theta table in LDS, since the other
 * contexts' ray passes fill this one's tail and idle slots).  Call before the first
 * reset / step.  Scheduling only: results are bit-identical with or without
 * it.  No reference counterpart (the reference steps one env per process). */
F110_API int f110_set_device_share(f110_ctx *ctx, int64_t device_cars, int32_t contexts);

/* ---- opponent policy -------------------------------------------------------
 * Replaces gap_follow_action (rl_training/utils/gap_follow.py:3-58), the
 * rule-based opponent train_ddpg.py:168 computes on the host each step from
 * the float32 info["scans"][1].  Device pointers: scan m is the n_beams
 * float32 values at scans + m*scan_stride (e.g. agent 1 of env m in
 * f110_outputs.scans: scans + B, stride A*B); its (steer, speed) goes to
 * actions[m*action_stride + 0/1] as float32 (e.g. agent 1's slot of the next
 * f110_step's action array: stride 2*A).  gaps [n_scans][2] (optional) gets
 * the chosen gap (start, end).  Bit-exact with the reference's NumPy
 * float32 arithmetic; angle_min / angle_increment are the reference
 * defaults -pi/2 and pi/1080 unless overridden.  Async on stream. */
F110_API int f110_gap_follow(const float *scans, int64_t n_scans, int64_t scan_stride, int32_t n_beams,
                             double angle_min, double angle_increment, float *actions, int64_t action_stride,
                             int32_t *gaps, void *stream);

/* ---- self-play ---------------------------------------------------------------
 * An opponent driven by a policy instead of gap_follow_action: the observation from its seat and
 * an actor head that writes into its rows of the next f110_step's action array.  No reference
 * counterpart (train_ddpg.py races the rule-based opponent only).  Device pointers, async on
 * `stream`; deterministic (no atomics). */

/* F110Env._pack_flat_obs (f110_env.py:552-584) as agent `agent` would see it:
 * out[e] = [ obs_scan(scans[e][agent][0..B)) , pose block of `agent`,
 *            pose blocks of the other agents in ascending index ]
 * The scan entries are the step's own (NaN / +inf -> lidar_max, -inf -> 0, clip to [0, lidar_max],
 * one f32 divide): agent == ego_idx reproduces the step's obs row bit for bit.  out must not
 * overlap obs.  16-byte accesses when n_beams and the three strides are multiples of 4 and the
 * pointers 16-byte aligned, 4-byte ones otherwise; the same values either way.  F110_E_INVALID:
 * agent outside [0, n_agents), a stride too small, a null pointer. */
F110_API int f110_agent_obs(const float *scans, int64_t scan_env_stride,      /* f110_outputs.scans, floats per env (>= A*B) */
                            const float *obs, int64_t obs_stride,             /* the step's obs: only its pose block [B, B+4A) is read */
                            int64_t n_envs, int32_t n_agents, int32_t n_beams, int32_t agent, float lidar_max,
                            float *out, int64_t out_stride, void *stream);    /* out_stride >= B + 4A */

/* act = shift + scale * tanh(h W^T + b) (Actor.forward's last line, agent.py:56-61) for the rows with
 * row_mask[i] != 0 (row_mask NULL: every row), written to out + i*out_stride; other rows of out untouched.
 * h [n_rows][K], W [nout][K], b / scale / shift [nout] as f110_ddpg_actor_head takes them; an
 * unmasked row gets the bits of that head's act.  No noise, no clip, no noise state:
 * choose_action(training=False) for those rows. */
F110_API int f110_policy_head_rows(const float *h, const float *W, const float *b, const float *scale, const float *shift,
                                   int64_t n_rows, int32_t K, int32_t nout, const uint8_t *row_mask,
                                   float *out, int64_t out_stride, void *stream);

/* ---- training reward ---------------------------------------------------------
 * Replaces rl_training/utils/rewards.py:CenterlineSafetyProgressReward
 * (:185-355) over utils/track_progress.py:CenterlineProgress (:5-110), the
 * reward train_ddpg.py:125-176 computes on the host from every next_obs.
 * Batched over envs on the device, one wave per env. */
typedef struct f110_track f110_track;

/* CenterlineProgress(csv, closed): xy [n][2] and the optional lane widths
 * (w_tr_right_m / w_tr_left_m, NULL = none) as the CSV holds them; arclength,
 * tangents, normals and segment midpoints are derived here exactly as the
 * reference derives them (track_progress.py:29-46).  Host pointers.
 * device < 0 builds the host arrays only (f110_track_arrays; no reward). */
F110_API int f110_track_create(f110_track **out, int32_t device, const double *xy, const double *w_right,
                               const double *w_left, int32_t n, int32_t closed);
F110_API int f110_track_destroy(f110_track *track);
/* The derived arrays (host copies; any pointer may be NULL): s [n],
 * tan/nrm/mid [n-1][2]; returns L (the total arclength). */
F110_API double f110_track_arrays(const f110_track *track, double *s, double *tan, double *nrm, double *mid);

/* CenterlineSafetyProgressReward.__init__ kwargs (rewards.py:196-230). */
typedef struct f110_reward_params {
    double dt, w_prog, forward_sign, alive_bonus, w_rel_lead, lead_clip, w_lat, lat_cap, default_half_width;
    double lidar_max, near_wall_dist, w_wall, wall_quantile, opp_safe_dist, w_opp, ego_crash_penalty;
    double opp_crash_bonus, beta;  /* beta: _Prog / _ProgFallback EMA factor (0.8) */
    int32_t grace_steps_wall, grace_steps_opp, auto_flip_steps; /* auto_flip_steps: _Prog (20) */
    int32_t use_progress;          /* 1: centerline _Prog (a track is given), 0: _ProgFallback */
} f110_reward_params;

/* Per-env reward state in device memory; all-zero bytes = reward_fn.reset()
 * (rewards.py:97-107 _Prog.reset, :256 reset). */
typedef struct f110_reward_state {
    double s_prev[2];  /* ego, opp: last arclength (_Prog._s_prev) */
    double px[2], py[2];  /* last positions (_p_prev / _ProgFallback.prev) */
    double cum[2];     /* _cum */
    double ema;        /* _ema_abs_dego / ma_ego */
    double t_last[2];  /* last lateral offsets */
    double auto_sum;   /* running sum of _auto_buf */
    int32_t steps;     /* _steps */
    int32_t auto_n;    /* len(_auto_buf) */
    int32_t flags;     /* bit0/1: s_prev ego/opp set, bit2/3: p_prev ego/opp set, bit4: _flip == -1 */
    int32_t pad_;
} f110_reward_state;

F110_API void f110_default_reward_params(f110_reward_params *p);

/* reward_fn(next_obs) for n_envs flat observations (device, float32
 * [n_envs][obs_len], the F110Env layout: n_beams scaled ranges, then x, y,
 * yaw, collision of ego and opponent; parse_flat_obs, rewards.py:11-41).
 * state: device [n_envs]; reset_mask: device [n_envs] u8 or NULL -- a
 * masked env's state is reset (reward_fn.reset()) and its reward is 0 (the
 * reset observation of an autoresetting vector env is not rewarded).
 * rewards: device [n_envs] f64.  track may be NULL when
 * params->use_progress == 0.  Async on stream. */
F110_API int f110_reward(const f110_track *track, const f110_reward_params *params, const float *obs, int64_t n_envs,
                         int32_t obs_len, int32_t n_beams, f110_reward_state *state, const uint8_t *reset_mask,
                         double *rewards, void *stream);

/* ---- pure-pursuit opponent ----------------------------------------------------
 * A waypoint follower on the track's centerline (the pure-pursuit planner of the upstream
 * f1tenth_gym examples; the reference races gap_follow_action only): a scripted driver that laps
 * the track at a chosen speed.  One car per row; everything in f64, a*b+c rounded twice:
 *   (s_proj, t, seg) = CenterlineProgress.project_xy(x, y)        -- f110_reward's projection, same bits
 *   sq = s_proj + direction*lookahead; closed track: if sq > L: sq -= L; if sq < 0: sq += L;
 *        open track: sq clamped to [0, L]
 *   i = searchsorted(s, sq, side="right") - 1 clipped to [0, n-2]
 *   u = (sq - s[i]) / (s[i+1] - s[i])  (0 for a zero-length segment); target = xy[i] + u*(xy[i+1] - xy[i])
 *   (dx, dy) = target - (x, y); d2 = dx*dx + dy*dy; ly = -sin(yaw)*dx + cos(yaw)*dy  (cr_sincos)
 *   kappa = 2*ly/d2; steer = clip(atan(wheelbase*kappa), -steer_limit, steer_limit)
 *   v = row_speed ? row_speed[m] : speed;
 *   a_lat > 0: v = min(max(sqrt(a_lat / max(|kappa|, 1e-9)), v_floor), v)   (a NaN |kappa| counts as 1e-9)
 *   d2 <= 1e-12: steer = 0 (v as computed);  a non-finite x, y or yaw: the action is (0, 0)
 * The only operation whose last bit a platform's libm may round differently is the f64 atan. */
typedef struct f110_pursuit_params {
    double lookahead;    /* m along the centerline (1.2); 0 < lookahead < L */
    double wheelbase;    /* lf + lr of f110_default_params (0.3302) */
    double speed;        /* m/s (4.0) */
    double a_lat;        /* m/s^2; 0: constant speed (the default), > 0: the curvature speed profile, which
                          * needs a car with v_min < 0 (the default car's PID turns braking into throttle) */
    double v_floor;      /* the profile's lowest speed (1.0) */
    double steer_limit;  /* rad (0.4189) */
    int32_t direction;   /* +1: ascending arclength, -1: descending */
    int32_t pad_;
} f110_pursuit_params;

F110_API void f110_default_pursuit_params(f110_pursuit_params *p);

/* Row m: pose (x, y, yaw) = the three float32 at poses + m*pose_stride (e.g. agent k's pose group of
 * the step's obs: obs + n_beams + 4*k, stride f110_outputs.obs_stride); (steer, v) as float32 to
 * actions[m*action_stride + 0/1] (e.g. agent k's slot of the next f110_step's action array: stride
 * 2*A).  row_speed: f64 [n_rows] or NULL (params->speed for all); row_mask: u8 [n_rows] or NULL as
 * f110_policy_head_rows takes it (rows with 0 keep their action and aux bytes); aux: f64 [n_rows][4]
 * or NULL, receives s_proj, t (a zero as +0), target_x, target_y (four NaNs for a non-finite pose).  Device
 * pointers; no allocation, no host synchronisation, no atomics (capturable); async on stream.
 * F110_E_INVALID: a null track / params / poses / actions, a host-only track, pose_stride < 3,
 * action_stride < 2, lookahead <= 0 or >= L, wheelbase <= 0, steer_limit <= 0, speed < 0,
 * a_lat < 0, a NaN among them, direction other than +1 / -1. */
F110_API int f110_pure_pursuit(const f110_track *track, const f110_pursuit_params *params, const float *poses,
                               int64_t n_rows, int64_t pose_stride, const double *row_speed,
                               const uint8_t *row_mask, float *actions, int64_t action_stride, double *aux,
                               void *stream);

/* ---- episode statistics (no reference counterpart: train_ddpg.py sums one
 * env's rewards in its Python loop) ------------------------------------------------
 * Per-env episode return and length of an autoresetting batch, and running
 * totals over the finished episodes, from each step's rewards and flags.  No
 * context; all pointers are device pointers; async on `stream`, no host
 * synchronisation and no allocation (capturable in a HIP graph).
 * Per env and call:
 *   was_reset:  ret = 0, len = 0, closed = 0, finished = 0; the row's reward is
 *               ignored (it is the reset observation of NEXT_STEP autoreset);
 *   closed:     the env ended and was not reset since (autoreset off): the row
 *               is ignored, finished = 0;
 *   otherwise:  ret += reward, len += 1; if terminated || truncated: finished =
 *               1, last_return = ret, last_length = len, closed = 1 and the env
 *               enters the totals, as terminated if terminated, else truncated;
 *               else finished = 0.
 * last_return / last_length keep their values where the env does not finish.
 * truncated, last_return, last_length and finished may be NULL.
 * Totals accumulate over calls (zero bytes = fresh; return_min / return_max are
 * meaningful only when episodes > 0).  The envs finishing in one call are
 * reduced in a fixed order: blocks of 256 consecutive envs reduce their (sum,
 * min, max, counts) in LDS as a binary tree over the env's position in the
 * block (entry i += entry i + h for h = 128, 64, .. 1; envs that do not finish
 * enter as +0.0), each block stores its partial to scratch, and a second
 * launch adds the partials in ascending block order, then that sum to the
 * totals.  No floating-point atomics: the same inputs give the same bits
 * whatever the timing.  scratch: f110_episode_scratch_bytes(n_envs) bytes. */
typedef struct f110_episode_state { double ret; int32_t len; int32_t closed; } f110_episode_state; /* zero bytes = fresh */
typedef struct f110_episode_totals { int64_t episodes, terminated, truncated, length_sum;
                                     double return_sum, return_min, return_max; } f110_episode_totals;
F110_API int64_t f110_episode_scratch_bytes(int64_t n_envs);
F110_API int f110_episode_stats(const double *rewards, const uint8_t *terminated, const uint8_t *truncated,
                                const uint8_t *was_reset, int64_t n_envs, f110_episode_state *state,
                                double *last_return, int32_t *last_length, uint8_t *finished,
                                f110_episode_totals *totals, void *scratch, void *stream);

/* ---- race statistics (no reference counterpart: train_ddpg.py reports returns only) ------------
 * Per-env race outcomes of an autoresetting batch -- the ego's progress along the centerline, its
 * lead over the opponent, passes made and suffered, how the episode ended -- and running totals
 * over the finished episodes, from each step's observations and flags.  No context; device
 * pointers; async on `stream`, no host synchronisation, no allocation, no atomics (capturable).
 * Everything is f64, evaluated left to right, no FMA apart from the projection's own.
 * Inputs per env e and call: the ego's pose group, four float32 (x, y, yaw, col) at ego + e*stride
 * (e.g. obs + n_beams + 4*ego_idx, stride f110_outputs.obs_stride), the opponent's at opp +
 * e*stride (opp == NULL: a single-agent env; there is no opponent part and lead, passes, passed
 * stay 0), and terminated, truncated (may be NULL), was_reset.  A car with finite x and y is
 * projected, (s_k, t_k) = CenterlineProgress.project_xy(x_k, y_k), the same function and bits as in
 * f110_reward and f110_pure_pursuit; a car with a non-finite x or y is "not ok" in this row.
 * wrap(d): on a closed track, if d > L/2: d -= L; if d < -L/2: d += L; on an open one d.
 * The rule, in this order:
 *   1. start row (was_reset != 0, or STARTED not set): the episode's first observation (NEXT_STEP
 *      autoreset's reset observation).  The state becomes zero, STARTED is set; for each ok car
 *      s_prev[k] = s_k and S_k is set; lead0 = wrap(direction*(s_0 - s_1)) if both cars are ok,
 *      else 0; AHEAD is set iff lead0 > 0.  terminated / truncated are ignored.  result = 0.
 *   2. closed row (CLOSED set: the env ended and was not reset since): ignored, result = 0.
 *   3. progress: for each ok car, if S_k is set: prog[k] += direction * wrap(s_k - s_prev[k]); then
 *      s_prev[k] = s_k and S_k is set (a car that is not ok keeps its s_prev).  len += 1.  If the
 *      ego is ok: t_max = max(t_max, |t_0|).
 *   4. lead and passes (with an opponent): col_1 != 0 sets OPP_CRASHED.  lead = lead0 + (prog[0] -
 *      prog[1]).  If AHEAD is clear and lead > pass_margin: AHEAD is set, passes += 1; else if
 *      AHEAD is set and lead < -pass_margin: AHEAD is cleared, passed += 1.
 *   5. finish (terminated || truncated): CLOSED is set; result = bit0 finished | bit1 ego crash
 *      (terminated && col_0 != 0) | bit2 completed (terminated && col_0 == 0: the lap toggles) |
 *      bit3 truncated (!terminated; terminated wins) | bit4 OPP_CRASHED | bit5 ahead at end
 *      (opponent present and lead > 0); last_progress = prog[0], last_lead = lead, last_length =
 *      len, and the env enters the totals with its counts, prog[0], lead, t_max, passes, passed.
 *   6. otherwise result = 0.
 * result is written every call; cur [n][2] (may be NULL) receives the state's progress prog[0] and
 * lead (lead0 + (prog[0] - prog[1]); 0 without an opponent) every call; the last_* arrays (may be
 * NULL) keep their values where the env does not finish.  Totals accumulate over calls (zero bytes
 * = fresh; progress_min / progress_max are meaningful only when episodes > 0; t_max is the largest
 * of the episodes' t_max).  The envs finishing in one call are reduced in f110_episode_stats'
 * order: blocks of 256 consecutive envs reduce their parts in LDS as a binary tree over the env's
 * position in the block (entry i += entry i + h for h = 128, 64, .. 1; envs that do not finish
 * enter as +0.0, or as nothing for min and max), each block stores its partial to scratch, and a
 * last launch adds the partials in ascending block order, then that sum to the totals.  The same
 * inputs give the same bits whatever the timing.  scratch: f110_race_scratch_bytes(n_envs) bytes
 * (the projections of the call and the block partials).
 * F110_E_INVALID: a null track / params / ego / terminated / was_reset / state / result / totals /
 * scratch, a host-only track, stride < 4, n_envs < 0, pass_margin negative or NaN, direction other
 * than +1 / -1. */
typedef struct f110_race_params {
    double pass_margin;  /* dead band of the lead, m (0.58, the car's length) */
    int32_t direction;   /* +1: ascending arclength, -1: descending */
    int32_t pad_;
} f110_race_params;
typedef struct f110_race_state {            /* zero bytes = fresh (not started) */
    double s_prev[2], prog[2];              /* ego, opp: last arclength; signed progress since the start row, m */
    double lead0, t_max;                    /* lead at the start row; largest |t| of the ego */
    int32_t len, passes, passed, flags;     /* flags: 1 STARTED, 2 CLOSED, 4 S0, 8 S1 (s_prev set), 16 AHEAD, 32 OPP_CRASHED */
} f110_race_state;
typedef struct f110_race_totals { int64_t episodes, ego_crashes, completed, truncated, opp_crashes, ahead_at_end,
                                  passes, passed, length_sum;
                                  double progress_sum, progress_min, progress_max, lead_sum, t_max; } f110_race_totals;
F110_API void f110_default_race_params(f110_race_params *p);
F110_API int64_t f110_race_scratch_bytes(int64_t n_envs);
F110_API int f110_race_stats(const f110_track *track, const f110_race_params *params, const float *ego, const float *opp,
                             int64_t stride, const uint8_t *terminated, const uint8_t *truncated,
                             const uint8_t *was_reset, int64_t n_envs, f110_race_state *state, double *cur,
                             double *last_progress, double *last_lead, int32_t *last_length, uint8_t *result,
                             f110_race_totals *totals, void *scratch, void *stream);

/* ---- track observation (no reference counterpart: _pack_flat_obs gives scaled ranges and map poses) --
 * A track-relative block of observation columns for one seat car `a` of every env, with an optional
 * other car `o` (-1: none): the seat's own dynamic state, its lateral offset and heading error on
 * the centerline, a preview of the centerline ahead in the car's frame and the other car's gap.
 * Meant to be appended after the step's n_beams + 4*n_agents columns (out = obs + n_beams +
 * 4*n_agents, out_stride = the obs row stride); off unless a caller asks for it.  Everything in
 * f64, left to right, a*b+c rounded twice; every column is stored as (float)value.
 *   width = f110_track_obs_width(n_preview, has_other) = 7 + 2*n_preview + (has_other ? 3 : 0),
 *           rounded up to a multiple of 4; the pad columns are written as +0.
 * One row, dir = (double)direction, L the track's length, n its node count:
 *   1. x, y, delta, v, yaw, yaw_rate, slip = the seat's state.  A non-finite x, y or yaw: all width
 *      columns are +0.
 *   2. (s_p, t, seg) = CenterlineProgress.project_xy(x, y)       -- f110_reward's projection, same bits
 *   3. i = min(seg, n-2)  (the projection's nearest-node fallback may return node n-1)
 *   4. (sn, cs) = cr_sincos(yaw);  5. (tx, ty) = dir * tan[i]
 *   6. c0 = v/v_scale, c1 = delta/steer_scale, c2 = yaw_rate/yaw_rate_scale, c3 = slip/slip_scale,
 *      c4 = dir*t/lat_scale
 *   7. c5 = sn*tx - cs*ty (sine of the heading error), c6 = cs*tx + sn*ty (its cosine)
 *   8. preview j < n_preview, d = preview[j]: sq = s_p + dir*d, wrapped once on a closed track (if
 *      sq > L: sq -= L; if sq < 0: sq += L), clamped to [0, L] on an open one; k = searchsorted(s,
 *      sq, side="right") - 1 clipped to [0, n-2]; u = (sq - s[k]) / (s[k+1] - s[k]) (0 for a
 *      zero-length segment); target = xy[k] + u*(xy[k+1] - xy[k]); (dx, dy) = target - (x, y);
 *      c[7+2j] = (cs*dx + sn*dy)/d, c[8+2j] = (-sn*dx + cs*dy)/d
 *   9. with another car, at columns 7 + 2*n_preview ..: a non-finite x_o or y_o gives three +0;
 *      otherwise (s_o, t_o) = project_xy(x_o, y_o), g = wrap(dir*(s_o - s_p)) (the race statistics'
 *      wrap: closed track, if g > L/2: g -= L; if g < -L/2: g += L), and the columns are
 *      clip(g/gap_scale, -1, 1), dir*(t_o - t)/lat_scale, (v_o - v)/v_scale
 *  10. the pad columns are +0.
 * No libm function beyond sqrt enters: the device and the host statement (f110_host_track_obs,
 * f110_debug.h) agree in every bit. */
typedef struct f110_track_obs_params {
    double v_scale;         /* m/s (20.0) */
    double steer_scale;     /* rad (0.4189) */
    double yaw_rate_scale;  /* rad/s (10.0) */
    double slip_scale;      /* rad (pi/3) */
    double lat_scale;       /* m (1.0) */
    double gap_scale;       /* m (10.0) */
    double preview[8];      /* m ahead along the centerline (1, 2, 4, 8); each used one in (0, L) */
    int32_t n_preview;      /* 0..8 (4) */
    int32_t direction;      /* +1: ascending arclength, -1: descending */
} f110_track_obs_params;

/* Host-only helpers.  f110_track_obs_width: the row's width in floats (a multiple of 4), or -1 for
 * n_preview outside 0..8. */
F110_API void f110_default_track_obs_params(f110_track_obs_params *p);
F110_API int32_t f110_track_obs_width(int32_t n_preview, int32_t has_other);

/* state: device [7][n_envs*n_agents] f64 in f110_get_state's layout (car a of env e at column
 * e*n_agents + a); out: device float32, row e at out + e*out_stride.  One wave per env; no
 * allocation, no host synchronisation, no atomics (capturable); async on stream.
 * F110_E_INVALID: a null or host-only track, null params / state / out, n_envs < 0, n_agents outside
 * 1..8, seat outside [0, n_agents), other neither -1 nor in [0, n_agents) or equal to seat,
 * out_stride < width, a scale that is not > 0, n_preview outside 0..8, a used preview distance not in
 * (0, L), direction other than +1 / -1; a NaN among them fails its test. */
F110_API int f110_track_obs(const f110_track *track, const f110_track_obs_params *params, const double *state,
                            int64_t n_envs, int32_t n_agents, int32_t seat, int32_t other, float *out,
                            int64_t out_stride, void *stream);
/* The same on the context's live state (n_envs, n_agents from the context): no copy is made and no
 * pointer leaves the library.  The track must be on the context's device. */
F110_API int f110_ctx_track_obs(f110_ctx *ctx, const f110_track *track, const f110_track_obs_params *params,
                                int32_t seat, int32_t other, float *out, int64_t out_stride, void *stream);

/* ---- scan observation (no reference counterpart: _pack_flat_obs hands the policy all 1080 ranges) --
 * A compact policy row made from the full observation row on the device: the range columns pooled
 * into sectors, the last few pooled frames stacked, the other columns carried through.  The full
 * rows stay what they are for everything else that reads them (the reward, the race statistics,
 * the opponents, the track observation's fill); off unless a caller asks for it.
 *   input row   [B range columns | M middle columns (the 4A pose groups) | T tail columns (the
 *               track block; may be 0)], float32, unit column stride, rows row_stride floats apart
 *   output row  [F*K | M if keep_mid | T], width = f110_scan_obs_width = F*K + keep_mid*M + T
 * One push of one env, K = n_bins, F = n_frames, S = stride, D = (F-1)*S + 1 (the ring depth):
 *   1. pooling: bin j < K covers beams [floor(j*B/K), floor((j+1)*B/K)) (64-bit integers; the bins
 *      may be ragged, K == B is the identity).  min: fminf over the bin, ascending.  mean: a float32
 *      sum over the bin in ascending beam order starting from the first beam's value, divided by
 *      (float)count -- IEEE division, no contraction.
 *   2. ring: per env D slots of K float32 and an int32 head, -1 = empty.  With head == -1 or the
 *      env's reset flag nonzero every slot takes the pooled frame and head becomes 0 (a refill);
 *      otherwise head becomes (head + 1) % D and that slot takes the pooled frame.
 *   3. output: frame j < F (0 = newest) is slot (head - j*S) mod D, at columns [j*K, (j+1)*K); the
 *      middle (if kept) and tail columns are the current input row's, not stacked.
 * All float32 and in a fixed order, so the device and the host statement (f110_host_scan_obs_push,
 * f110_debug.h) agree in every bit.  Limits (by design): 1 <= K <= B <= 4096, 1 <= F <= 8,
 * 1 <= S <= 16, D <= 32. */
typedef struct f110_scan_obs f110_scan_obs;
typedef struct f110_scan_obs_params {
    int32_t n_bins;    /* K: pooled sectors, 1..n_beams (108) */
    int32_t n_frames;  /* F: stacked frames, 1..8 (1) */
    int32_t stride;    /* S: simulator steps between stacked frames, 1..16 (1) */
    int32_t reduce;    /* 0 = min (default), 1 = mean */
    int32_t keep_mid;  /* 1: carry the middle columns (default), 0: drop them */
} f110_scan_obs_params;

/* Host-only helpers.  f110_scan_obs_width: the output row's width in floats, or -1 for parameters
 * or a shape f110_scan_obs_create would refuse. */
F110_API void f110_default_scan_obs_params(f110_scan_obs_params *p);
F110_API int32_t f110_scan_obs_width(const f110_scan_obs_params *params, int32_t n_beams, int32_t n_mid,
                                     int32_t n_tail);

/* The ring [n_envs][D][K] float32 and the heads [n_envs] int32 (all -1) on `device`.
 * F110_E_INVALID: a null pointer, n_envs < 1, a shape or parameter outside the limits above. */
F110_API int f110_scan_obs_create(f110_scan_obs **out, int32_t device, int64_t n_envs, int32_t n_beams,
                                  int32_t n_mid, int32_t n_tail, const f110_scan_obs_params *params);
F110_API int f110_scan_obs_destroy(f110_scan_obs *so);
/* One push of every env: rows / out device float32 (row e at rows + e*row_stride, out + e*out_stride),
 * reset device u8 [n_envs] or NULL (no env resets).  One launch, one wave per env; the head is on
 * the device: no allocation, no host synchronisation, no atomics (capturable); async on stream.
 * F110_E_INVALID: a null pointer, row_stride < B + M + T, out_stride < width, out overlapping rows. */
F110_API int f110_scan_obs_push(f110_scan_obs *so, const float *rows, int64_t row_stride, const uint8_t *reset,
                                float *out, int64_t out_stride, void *stream);
/* Empties the rings (head = -1) of the envs with env_mask != 0; the next push refills them. */
F110_API int f110_scan_obs_reset(f110_scan_obs *so, const uint8_t *env_mask /* NULL = all */, void *stream);
/* The device ring and heads (tests); either may be NULL. */
F110_API int f110_scan_obs_arrays(f110_scan_obs *so, float **ring, int32_t **head);

/* ---- sensor randomization (no reference counterpart: the reference's scan noise is one std for
 *      every env, and its poses are exact) ---------------------------------------------------------
 * The third leg of the domain randomization, beside f110_set_param_randomization (the car) and
 * f110_set_spawn_randomization (the start state): the full observation row turned into the row the
 * policy, the replay and the critic see, under sensor parameters drawn per env and episode on the
 * device.  Everything else that reads the observation (the reward, the statistics, the opponents)
 * keeps the clean row; off unless a caller asks for it.
 *   row  [B range columns | M middle columns (4 per agent: x, y, theta, collision) | T tail columns],
 *        float32, unit column stride; the output row has the same width and layout
 * Each parameter is uniform in its (lo, hi) pair; f110_default_sensor_params is the identity:
 *   scale       multiplicative range error                                             (1, 1)
 *   noise_abs   additive range noise sigma, metres                                     (0, 0)
 *   noise_rel   range-proportional noise sigma, a fraction of the range                (0, 0)
 *   dropout     per-beam, per-step probability of no return (the beam reads max range) (0, 0)
 *   blackout    width in whole beams of one contiguous blocked sector (it reads 0); its first beam
 *               is drawn once per episode, uniform over [0, B - width]                  (0, 0)
 *   quant       range quantization step, metres; 0 = off                               (0, 0)
 *   pose_xy     sigma of the noise on every x and y column, metres                     (0, 0)
 *   pose_theta  sigma of the noise on every theta column, radians                      (0, 0)
 * Counters, per env on the device: episode (-1 = no apply yet) and step.  An apply of an env with
 * episode < 0 or a nonzero reset flag starts an episode: episode = (episode + 1) mod 2^31, step = 0
 * and the parameter row is redrawn; any other apply has step = step + 1 (mod 2^32).
 * Draws: Philox4x32-10 (csrc/f110_rng.h) under the key of f110_set_param_randomization,
 *   k0 = (u32)seed ^ (u32)g, k1 = (u32)(seed >> 32) ^ (u32)(g >> 32) ^ 0xA5A5A5A5, g = env_offset + e
 * (the global env id: nothing depends on n_envs, the launch shape or the sharding over ranks).
 *   parameter block j < 3: counter (j, 0, 0x5E250, episode); block 0 = scale, noise_abs, noise_rel,
 *     dropout; block 1 = blackout width, blackout start, quant, pose_xy; block 2 word 0 = pose_theta.
 *     A real parameter is lo + u * (hi - lo), u = (float)(word >> 8) * 2^-24; the width is
 *     lo + mulhi(word, hi - lo + 1), the start mulhi(word, B - width + 1), mulhi(w, n) = (w * n) >> 32
 *     in 64 bits.  noise_abs and quant are then divided by range_max (the row's units), once;
 *     the dropout threshold is (u32)(dropout * 2^24).
 *   column block: counter (column, step, 0x5E251, episode), column = b for beam b, B + m for middle
 *     column m.  z = (float)(S - 1530) * (1/256) with S the sum of the 12 bytes of words 0..2 (mean
 *     0, std sqrt(65535)/256, |z| < 5.98); the dropout bits are word 3 >> 8.
 * One beam of value d, all float32, in this order, no contraction:
 *   1. d = d * scale
 *   2. if noise_abs_n > 0 or noise_rel > 0:  d = d + z * (noise_abs_n + noise_rel * d)
 *   3. if quant_n > 0:  d = quant_n * rintf(d / quant_n)
 *   4. if the beam's 24 dropout bits < the threshold:  d = 1
 *   5. if start <= b < start + width:  d = 0
 *   6. d < 0 gives 0, d > 1 gives 1
 * One pose column of value v: x and y with pose_xy > 0 become v + z * pose_xy; theta with
 * pose_theta > 0 becomes t = v + z * pose_theta, then t - 2pi if t > pi, t + 2pi if t < -pi (float32
 * pi and 2pi).  Collision columns, the tail and columns whose sigma is 0 keep their bits; so the
 * identity parameters return a row of ranges in [0, 1] bit for bit.
 * An env whose env_mask byte is 0 is copied through unchanged; its counters and parameter row advance
 * all the same (a trainer's noise-free evaluation envs).
 * The device and the host statement (f110_host_sensor_apply, f110_debug.h) agree in every bit.
 * Limits (by design): 1 <= B <= 4096, M a multiple of 4. */
typedef struct f110_sensor f110_sensor;
typedef struct f110_sensor_params {  /* (lo, hi) each */
    float scale[2];
    float noise_abs[2];
    float noise_rel[2];
    float dropout[2];
    float blackout[2];
    float quant[2];
    float pose_xy[2];
    float pose_theta[2];
} f110_sensor_params;

F110_API void f110_default_sensor_params(f110_sensor_params *p);

/* The parameter rows [n_envs][10] float32 (scale, noise_abs / range_max, noise_rel, dropout, blackout
 * width, blackout start, quant / range_max, pose_xy, pose_theta, dropout threshold), zeros, and the
 * counters [n_envs] int32 (episode -1, step 0) on `device`.  env_mask: HOST u8 [n_envs] copied to the
 * device, or NULL (every env is touched).  range_max: what the range columns were divided by (the
 * context's lidar_max).
 * F110_E_INVALID, the argument named, before any device call: a null out or params, n_envs < 1, n_beams
 * outside [1, 4096], n_mid not a multiple of 4, n_mid or n_tail negative, range_max not > 0,
 * env_offset < 0, a bound that is not finite, lo > hi, scale <= 0, a negative sigma or quant, dropout
 * outside [0, 1], blackout outside [0, n_beams] or not whole. */
F110_API int f110_sensor_create(f110_sensor **out, int32_t device, int64_t n_envs, int32_t n_beams, int32_t n_mid,
                                int32_t n_tail, float range_max, uint64_t seed, int64_t env_offset,
                                const uint8_t *env_mask, const f110_sensor_params *params);
F110_API int f110_sensor_destroy(f110_sensor *sn);
/* One apply of every env: rows / out device float32 (row e at rows + e*row_stride, out + e*out_stride),
 * reset device u8 [n_envs] or NULL (no env resets).  out is rows itself (same pointer and stride) or
 * shares no float with it.  One launch, one block per env; the counters and the parameter rows are on
 * the device: no allocation, no host synchronisation, no atomics (capturable); async on stream.
 * F110_E_INVALID: a null pointer, row_stride or out_stride below B + M + T, out overlapping rows in
 * part. */
F110_API int f110_sensor_apply(f110_sensor *sn, const float *rows, int64_t row_stride, const uint8_t *reset,
                               float *out, int64_t out_stride, void *stream);
/* Restarts the counters (episode = -1, step = 0) of the envs with env_mask != 0 (device u8): their
 * next apply starts episode 0 again. */
F110_API int f110_sensor_reset(f110_sensor *sn, const uint8_t *env_mask /* NULL = all */, void *stream);
/* The device parameter rows and counters (tests); any may be NULL. */
F110_API int f110_sensor_arrays(f110_sensor *sn, float **param_rows, int32_t **episode, int32_t **step);

/* ---- prioritized experience replay ---------------------------------------------
 * Replaces rl_training/DDPG/replay_buffer.py:PrioritizedExperienceReplayBuffer
 * (:6-135), the DDPG agent's memory (agent.py:194): a ring of transitions
 * (state, action, reward, next_state, done) with one float32 priority each.
 * All of it lives in device memory; every call below is asynchronous on
 * `stream` and takes device pointers, except f110_replay_length /
 * f110_replay_stats and the test hooks f110_replay_select_keys /
 * f110_replay_select_state, which wait for the stream. */
typedef struct f110_replay f110_replay;

/* PrioritizedExperienceReplayBuffer(buffer_size=capacity, batch_size, alpha,
 * seed, priority_epsilon=eps) (:18-40).  max_batch bounds the batch of
 * f110_replay_sample (<= 8192) and max_add the rows of one f110_replay_add;
 * obs_dim / act_dim are the state / action lengths (1088 / 2 in train_ddpg). */
F110_API int f110_replay_create(f110_replay **out, int32_t device, int64_t capacity, int32_t obs_dim,
                                int32_t act_dim, int32_t max_batch, int64_t max_add, double alpha, double eps,
                                uint64_t seed);
F110_API int f110_replay_destroy(f110_replay *rb);

/* n calls of add(Experience(state, action, reward, next_state, done)) with
 * priority=None (:48-71, agent.remember agent.py:223-237), in row order: the
 * new rows get the current max priority (1.0 when empty).  obs / next_obs:
 * rows of obs_dim floats at a stride of obs_stride / next_stride floats;
 * act: act_dim floats per row at act_stride; reward [n] f32; done [n] u8
 * (NULL = all 0).  priority [n] f32: add(exp, priority=p) (clipped to
 * [1e-8, FLT_MAX]); NULL = priority=None.  mask [n] u8 (NULL = all rows):
 * only rows with mask != 0 are stored (e.g. not the reset rows of an
 * autoresetting vector env). */
F110_API int f110_replay_add(f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                             int64_t act_stride, const float *reward, const float *next_obs, int64_t next_stride,
                             const uint8_t *done, const float *priority, const uint8_t *mask, int64_t n,
                             void *stream);

/* f110_replay_add for a vector env's raw step outputs (train_ddpg.py:177-183,
 * agent.remember per transition): reward [n] f64 (stored rounded to f32),
 * terminated [n] u8 (the done flag), was_reset [n] u8 -- rows with
 * was_reset != 0 (NEXT_STEP autoreset: obs is the finished episode's, next_obs
 * the new one's) are not stored.  No torch dtype conversions on the caller's side. */
F110_API int f110_replay_add_env(f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                                 int64_t act_stride, const double *reward, const float *next_obs,
                                 int64_t next_stride, const uint8_t *terminated, const uint8_t *was_reset,
                                 int64_t n, void *stream);

/* sample(beta) (:76-116) of `batch` rows: without replacement when the buffer
 * holds at least `batch` rows (distributed like numpy's
 * Generator.choice(replace=False, p=...): successive draws, in draw order),
 * i.i.d. otherwise.  Writes idx [batch] i64, weights [batch] f32 (normalised
 * IS weights) and, when obs != NULL, the gathered batch agent.replay stacks
 * (agent.py:257-270): obs / next_obs [batch][obs_dim], act [batch][act_dim],
 * reward / done [batch] f32.  The caller must not sample an empty buffer
 * (the reference raises ValueError, :83-84). */
F110_API int f110_replay_sample(f110_replay *rb, int32_t batch, double beta, int64_t *idx, float *weights, float *obs,
                                float *act, float *reward, float *next_obs, float *done, void *stream);

/* Test hook: f110_replay_sample's selection and weights over keys the caller
 * chooses in place of the drawn ones, with no gather.  keys [n] u32 (device;
 * the float32 patterns of the exponential-race keys lie in [0, 0x7F800000]),
 * n == the buffer's length (the call waits for `stream` to read it) and
 * batch <= n.  Selects the batch smallest by (key, index): idx [batch] in
 * ascending order, weights as f110_replay_sample.  Counts as one sample (the
 * next draw differs). */
F110_API int f110_replay_select_keys(f110_replay *rb, const uint32_t *keys, int64_t n, int32_t batch, double beta,
                                     int64_t *idx, float *weights, void *stream);

/* update_priorities(idx, priorities) (:121-135): the priority of row idx[j]
 * becomes clip(p_j, 1e-8, FLT_MAX) in float32 with NaN -> 1e-6, where
 * p_j = values[j] (from_td == 0) or agent.replay's |values[j]| + add_eps
 * (from_td != 0, values = TD errors, agent.py:337).  Repeated indices keep
 * the last value. */
F110_API int f110_replay_update_priorities(f110_replay *rb, const int64_t *idx, const float *values, int64_t n,
                                           int32_t from_td, float add_eps, void *stream);

/* len(buffer) (:42-43) and the ring pointer; waits for `stream`. */
F110_API int f110_replay_length(f110_replay *rb, int64_t *length, int64_t *next_idx, void *stream);

/* Device pointers of the stored arrays (read-only views for tests and
 * checkpoints): priority [capacity] f32, obs / next_obs [capacity][obs_dim],
 * act [capacity][act_dim], reward / done [capacity] f32.  Any out pointer
 * may be NULL. */
F110_API int f110_replay_arrays(f110_replay *rb, float **priority, float **obs, float **act, float **reward,
                                float **next_obs, float **done);

/* The last sample's select (read-only, for tests): the device pointers of its
 * keys [capacity] u32 and of the sampling weights (priority + eps)^alpha
 * [capacity] f64, and a host copy (waits for `stream`) of the threshold key
 * (prefix), the rows still to take among the keys equal to it (kleft), the
 * rows below it (n_lt), the sum of the weights (den) and the count of samples
 * that met more equal keys at the threshold than the tie list holds
 * (overflow).  Any out pointer may be NULL. */
F110_API int f110_replay_select_state(f110_replay *rb, uint32_t **keys, double **wt, uint32_t *prefix,
                                      uint32_t *kleft, uint32_t *n_lt, double *den, uint32_t *overflow,
                                      void *stream);

/* ---- n-step returns (no reference counterpart: agent.replay's targets are one-step) --
 * An accumulator in front of the replay ring: per env a window of at most n_step
 * pending entries (obs, act, a running return ret in f64, a reward count k),
 * oldest first, and a power table pw[i] = gamma^i (f64, sequential products,
 * pw[0] = 1).  One f110_nstep_push takes n_envs raw step outputs, as
 * f110_replay_add_env does.  Per env:
 *   was_reset != 0:  the window is dropped, nothing is emitted (a NEXT_STEP reset
 *                    row; after an ending step the window is already empty);
 *   otherwise:       every pending entry, oldest first: ret = ret + pw[k] * r,
 *                    k += 1 (product and sum rounded separately); then
 *                    (s, a, ret = r, k = 1) is appended;
 *     terminated || truncated:  every entry is emitted, oldest first, with done =
 *                    1.0f if terminated, else (float)(1.0 - pw[k - 1]); the window
 *                    is empty afterwards;
 *     else, n_step entries pending:  the oldest is emitted with done =
 *                    (float)(1.0 - pw[n_step - 1]).
 * An emitted row is (obs, act of the entry, (float)ret, this push's next_obs,
 * done).  The done column is the effective done d_eff = 1 - gamma^(k-1) (1 - done):
 * every TD target here is r + gamma * (1 - d) * q with d in float32, so the stored
 * row bootstraps with gamma^k (1 - done) through the one-step kernels.  With
 * n_step = 1 a push stores exactly f110_replay_add_env's rows.
 * The emitted rows of one push are appended by env ascending, oldest first within
 * an env, each with the ring's current max priority: what that many
 * f110_replay_add rows (priority NULL) in this order would store.  Async on
 * `stream`, no host read and no allocation after create (capturable in a HIP
 * graph).  1 <= n_step <= 16, gamma finite in [0, 1]; at push obs_dim / act_dim
 * must equal the replay's and n_envs * n_step must not exceed its capacity (its
 * max_add does not apply).  truncated may be NULL (all 0).  The windows take
 * n_step * n_envs * (obs_dim + act_dim) * 4 bytes. */
typedef struct f110_nstep f110_nstep;
F110_API int f110_nstep_create(f110_nstep **out, int32_t device, int64_t n_envs, int32_t n_step, double gamma,
                               int32_t obs_dim, int32_t act_dim);
F110_API int f110_nstep_destroy(f110_nstep *ns);
F110_API int f110_nstep_push(f110_nstep *ns, f110_replay *rb, const float *obs, int64_t obs_stride, const float *act,
                             int64_t act_stride, const double *reward, const float *next_obs, int64_t next_stride,
                             const uint8_t *terminated, const uint8_t *truncated, const uint8_t *was_reset,
                             void *stream);
/* Drops the windows of the envs with env_mask != 0 (NULL = all); emits nothing. */
F110_API int f110_nstep_reset(f110_nstep *ns, const uint8_t *env_mask /* NULL = all */, void *stream);
/* Device views for tests: len / head [n_envs] (entry i of env e sits in slot
 * (head + i) % n_step), ret / k [n_envs][n_step], obs [n_envs][n_step][obs_dim],
 * act [n_envs][n_step][act_dim].  Any out pointer may be NULL. */
F110_API int f110_nstep_arrays(f110_nstep *ns, int32_t **len, int32_t **head, double **ret, int32_t **k,
                               float **obs, float **act);

/* ---- action repeat (no reference counterpart: agent.act runs at every simulator step) --
 * A control interval of `repeat` simulator steps around the env step: the policy's
 * action is held for a block of up to `repeat` steps and the block is stored as ONE
 * replay row.  An f110_repeat handle holds per env a phase k (int32; 0: a decision is
 * due), a running return ret (f64), the block's first observation s_obs[obs_dim] and
 * its action s_act[act_dim] (f32), and a power table pw[i] = gamma^i (f64, sequential
 * products, pw[0] = 1, as the n-step table).
 * f110_repeat_hold runs BEFORE the env step.  Per env:
 *   k == 0:  s_obs = the obs row, s_act = the act row, decision = 1; the act row stays
 *            as the policy wrote it;
 *   k > 0:   the act row = s_act, decision = 0.
 * f110_repeat_push runs AFTER the env step.  Per env:
 *   was_reset != 0:  k = 0, nothing is emitted (a NEXT_STEP reset row, or an env reset
 *                    from outside mid-block: the block is dropped, as the n-step
 *                    window is);
 *   otherwise:       ret = (k == 0) ? r : ret + pw[k] * r (product and sum rounded
 *                    separately; a lone -0.0 survives), k += 1; then, if terminated ||
 *                    truncated || k == repeat, the row (s_obs, s_act, (float)ret, this
 *                    push's next_obs row, done) is emitted with done = 1.0f if
 *                    terminated, else (float)(1.0 - pw[k - 1]), and k = 0.
 * The done column is the effective done of the n-step section, so the one-step TD
 * kernels bootstrap a block of k steps with gamma^k.  Envs keep their own phase: an
 * episode that ends mid-block ends the block, and the env's next decision is due at
 * the first step of its next episode.
 * The emitted rows of one push are appended by env ascending, each with the ring's
 * current max priority: what one f110_replay_add (priority NULL) of those rows would
 * store.  With repeat == 1 a hold changes no action and a push stores exactly
 * f110_replay_add_env's rows.  Async on `stream`, no host read and no allocation
 * after create (capturable in a HIP graph); hold and push of one handle must be
 * issued on one stream (the next hold overwrites the rows a push reads).
 * 1 <= repeat <= 64, gamma finite in [0, 1], n_envs >= 1; at push obs_dim / act_dim
 * must equal the replay's and n_envs must not exceed its capacity (its max_add does
 * not apply).  decision (u8 [n_envs]) and truncated may be NULL.  The handle takes
 * n_envs * (obs_dim + act_dim) * 4 bytes plus the small per-env arrays. */
typedef struct f110_repeat f110_repeat;
F110_API int f110_repeat_create(f110_repeat **out, int32_t device, int64_t n_envs, int32_t repeat, double gamma,
                                int32_t obs_dim, int32_t act_dim);
F110_API int f110_repeat_destroy(f110_repeat *rp);
F110_API int f110_repeat_hold(f110_repeat *rp, const float *obs, int64_t obs_stride, float *act /* in/out */,
                              int64_t act_stride, uint8_t *decision /* [n_envs], may be NULL */, void *stream);
F110_API int f110_repeat_push(f110_repeat *rp, f110_replay *rb, const double *reward, const float *next_obs,
                              int64_t next_stride, const uint8_t *terminated, const uint8_t *truncated,
                              const uint8_t *was_reset, void *stream);
/* Sets k = 0 for the envs with env_mask != 0 (NULL = all); emits nothing. */
F110_API int f110_repeat_reset(f110_repeat *rp, const uint8_t *env_mask /* NULL = all */, void *stream);
/* Device views for tests: k [n_envs], ret [n_envs], obs [n_envs][obs_dim],
 * act [n_envs][act_dim].  Any out pointer may be NULL. */
F110_API int f110_repeat_arrays(f110_repeat *rp, int32_t **k, double **ret, float **obs, float **act);

/* ---- learner optimizer ----------------------------------------------------------
 * One torch.optim.Adam step (agent.py:187-188: Adam(params, lr), betas
 * (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) over a network whose
 * parameters, gradients and moments are flat float32 device buffers of n
 * elements.  state: device int64 step counter followed by a uint32 scratch
 * word (both zero initially); the step is advanced on the device, so the
 * call can be captured in a HIP graph.  target (may be null): the network's
 * target copy, soft-updated in the same pass after the step (agent.py:340-341,
 * target.lerp_(param, tau)).  Async on stream. */
F110_API int f110_adam_step(float *param, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t n, double lr,
                            double beta1, double beta2, double eps, void *state, float *target, double tau,
                            void *stream);

/* ---- learner heads -------------------------------------------------------------
 * The DDPG networks' output layers fused with what follows them
 * (rl_training agent.py: Actor.fc3 + tanh + action-box map :56-61, Critic.q
 * :93-97, replay()'s TD target :302-308, weighted MSE :310-316, actor loss
 * -mean(q) :321-326), replacing torch's skinny GEMM + elementwise launches.
 * Row-major float32 device buffers: h [B][K] (the last hidden layer), W
 * [nout][K], b [nout]; K <= 255, nout <= 4 (nout = 1 for the critic).
 * scratch: f110_ddpg_scratch_floats(B, K, nout) floats.  dh / dW / db
 * outputs may be null (not wanted); dh_mask [B][K] (may be null) zeroes dh
 * where dh_mask <= 0 (h's ReLU: threshold_backward fused into the head).  g: device scalar, the gradient of the
 * loss (autograd's grad_output).  Deterministic; async on stream. */
F110_API int64_t f110_ddpg_scratch_floats(int32_t B, int32_t K, int32_t nout);
/* t = tanh(h W^T + b); act = scale * t + shift  (act, t: [B][nout]) */
F110_API int f110_ddpg_actor_head(const float *h, const float *W, const float *b, const float *scale,
                                  const float *shift, int32_t B, int32_t K, int32_t nout, float *act, float *t,
                                  void *stream);
/* choose_action(training=True) after the hidden layers (agent.py:350-370 with
 * GaussianActionNoise :520-539): out[row * out_stride + j] = clip(scale * tanh(h W^T + b) + shift
 * + sigma * n, low[j], high[j]), n ~ N(0, 1) independent per (row, j) and per call (Philox2x32
 * keyed by seed, counter = the call index); NaN actions stay NaN.  The noise state lives on the
 * device so a captured graph can replay the call: state_in = {sigma, call index} (f64), and the
 * launch writes state_out = {max(sigma * decay, sigma_min), call index + 1} (state_out !=
 * state_in: callers alternate two slots).  out may be a strided view (e.g. the vector env's
 * action rows). */
F110_API int f110_ddpg_actor_explore(const float *h, const float *W, const float *b, const float *scale,
                                     const float *shift, int32_t B, int32_t K, int32_t nout, const double *state_in,
                                     double *state_out, double decay, double sigma_min, const float *low,
                                     const float *high, uint64_t seed, float *out, int64_t out_stride, void *stream);
/* f110_ddpg_actor_explore per row: a batch whose rows are envs, some exploring and some evaluating,
 * with GaussianActionNoise (kind 0) or OUActionNoise (kind 1, agent.py:469-505).  The leading
 * arguments, the (sigma, call index) pair and its decay are f110_ddpg_actor_explore's; act below is
 * scale[j] * tanh(z) + shift[j], f110_ddpg_actor_head's value bit for bit.  Per row r, output j:
 *  - reset[r] != 0 (reset: [B] u8 or NULL) zeroes the row's ou_x first -- on every row, eval rows too;
 *  - eval_mask[r] != 0 ([B] u8 or NULL): out = act, unclipped, no draw used, ou_x untouched
 *    (`if not training: return action`);
 *  - the draw n = normals_ext[r * nout + j] (normals_ext: [B][nout] f32 caller-supplied N(0,1), or
 *    NULL), else f110_ddpg_actor_explore's own draw for (seed, call index, r, j): keys are by row, so
 *    eval rows do not shift the other rows' draws;
 *  - kind 0: out = clip(act + (float)sigma * n, low[j], high[j]) in f32, f110_ddpg_actor_explore's
 *    operations (with reset, eval_mask and normals_ext NULL the two entry points agree bit for bit);
 *  - kind 1: in f64, left to right, no FMA, with x = ou_x[r][j] (ou_x: [B][nout] f64, read and
 *    written; required):  dx = theta * (mu - x) * dt + (sigma * sqrt(dt)) * (double)n;  x' = x + dx,
 *    stored back;  out = (float)clip((double)act + x', (double)low[j], (double)high[j]).  This is
 *    OUActionNoise.__call__ as NumPy evaluates it (a float64 state after the first call, a float32
 *    draw) for mu = 0, the only value the reference constructs.
 * NaN stays NaN.  state_out is written once per launch whatever the masks hold: a caller with no
 * exploring row uses f110_ddpg_actor_head.  F110_E_INVALID before any device call for kind outside
 * {0, 1}, kind 1 without ou_x, dt < 0, a non-finite theta / mu / dt, state_in == state_out, or a bad
 * shape (K <= 255, nout <= 4, B > 0). */
F110_API int f110_ddpg_actor_explore_env(const float *h, const float *W, const float *b, const float *scale,
                                         const float *shift, int32_t B, int32_t K, int32_t nout,
                                         const double *state_in, double *state_out, double decay, double sigma_min,
                                         const float *low, const float *high, uint64_t seed, float *out,
                                         int64_t out_stride, int32_t kind, double *ou_x, double theta, double mu,
                                         double dt, const uint8_t *reset, const uint8_t *eval_mask,
                                         const float *normals_ext, void *stream);
/* The critic update's head in one launch: y = r + gamma (1 - d) (ht Wt^T + bt) (the target critic),
 * td = y - (h W^T + b), part[blk] = block sums of w td^2 (f110_ddpg_row_blocks(B) floats; the loss
 * is sum(part) / B: f110_learner_wgrad_loss), dq = -((g / B) w) (2 td) (may be null), dh = dq W where
 * dh_mask > 0 (dh may be null).  = f110_ddpg_td_target + f110_ddpg_critic_loss + the row part of
 * f110_ddpg_critic_loss_bwd, same float operations. */
F110_API int f110_ddpg_critic_step(const float *ht, const float *Wt, const float *bt, const float *r, const float *d,
                                   float gamma, const float *h, const float *W, const float *b, const float *w,
                                   const float *g, int32_t B, int32_t K, float *td, float *dh, const float *dh_mask,
                                   float *dq, float *part, void *stream);
/* The actor update's loss head: part[blk] = block sums of q = h W^T + b (the loss is sign sum(part) / B),
 * dh = (sign g / B) W where dh_mask > 0.  = f110_ddpg_q_mean + the row part of f110_ddpg_q_mean_bwd. */
F110_API int f110_ddpg_q_mean_step(const float *h, const float *W, const float *b, const float *g, float sign,
                                   int32_t B, int32_t K, float *dh, const float *dh_mask, float *part, void *stream);
/* blocks of the row-per-half-wave head launches for B rows (their partial-sum counts) */
F110_API int32_t f110_ddpg_row_blocks(int32_t B);
/* dz = (dact * scale) * (1 - t*t); dh = dz W; dW = dz^T h; db = sum_rows dz */
F110_API int f110_ddpg_actor_head_bwd(const float *h, const float *W, const float *t, const float *scale,
                                      const float *dact, int32_t B, int32_t K, int32_t nout, float *dh,
                                      const float *dh_mask, float *dW, float *db, float *scratch, void *stream);
/* y = r + (gamma * (1 - d)) * (h W^T + b) */
F110_API int f110_ddpg_td_target(const float *h, const float *W, const float *b, const float *r, const float *d,
                                 float gamma, int32_t B, int32_t K, float *y, void *stream);
/* td = y - (h W^T + b); loss = mean(w * td * td)  (loss: device scalar) */
F110_API int f110_ddpg_critic_loss(const float *h, const float *W, const float *b, const float *y, const float *w,
                                   int32_t B, int32_t K, float *td, float *loss, float *scratch, void *stream);
/* dq = -((g / B) * w) * (2 td); dh, dW, db from dq */
F110_API int f110_ddpg_critic_loss_bwd(const float *h, const float *W, const float *td, const float *w,
                                       const float *g, int32_t B, int32_t K, float *dh, const float *dh_mask,
                                       float *dW, float *db, float *scratch, void *stream);
/* loss = sign * mean(h W^T + b)  (sign -1: the actor loss) */
F110_API int f110_ddpg_q_mean(const float *h, const float *W, const float *b, float sign, int32_t B, int32_t K,
                              float *loss, float *scratch, void *stream);
/* A hidden layer's ReLU backward with its bias gradient (agent.py's F.relu(fc(x))
 * under autograd): gz = gy where y > 0 else 0 (torch threshold_backward), db =
 * sum_rows gz (db may be null).  gy, y, gz: [B][K]; K <= 1024; scratch:
 * f110_ddpg_relu_bwd_scratch_floats(B, K) floats. */
F110_API int64_t f110_ddpg_relu_bwd_scratch_floats(int32_t B, int32_t K);
F110_API int f110_ddpg_relu_bwd(const float *gy, const float *y, int32_t B, int32_t K, float *gz, float *db,
                                float *scratch, void *stream);
/* dq = sign * (g / B); dh, dW, db from dq (h only needed for dW / db) */
F110_API int f110_ddpg_q_mean_bwd(const float *h, const float *W, const float *g, float sign, int32_t B, int32_t K,
                                  float *dh, const float *dh_mask, float *dW, float *db, float *scratch,
                                  void *stream);

/* ---- TD3 heads -------------------------------------------------------------------
 * The two heads the TD3 update rule (clipped double-Q, target-policy smoothing) adds to the learner
 * heads above; same buffers, shapes and limits (K <= 255, nout <= 4, B > 0), f32 left to right
 * without FMA in the epilogues, deterministic, async on stream.
 *
 * f110_td3_target_action: the target actor's output layer with smoothing.  act = scale[j] *
 * tanh(h W^T + b) + shift[j] is f110_ddpg_actor_head's value bit for bit; per row r, output j
 *   s = policy_noise * scale[j];  c = noise_clip * scale[j];  e = clip(s * n, -c, c);
 *   out[r][j] = clip(act + e, low[j], high[j])        (out: [B][nout], packed)
 * so policy_noise and noise_clip are in units of the tanh output (scale = the actor's half-range
 * 0.5 (high - low)).  The draw n is normals_ext[r * nout + j] when normals_ext ([B][nout] f32) is
 * given, else f110_ddpg_actor_explore's Philox / Box-Muller draw for (seed ^ a fixed 64-bit tag,
 * *counter, r, j): a stream of its own, never the exploration stream's for the same (seed, counter,
 * row).  counter is a device int64 the launch only reads -- the learner passes the critic
 * optimizer's step word (f110_adam_step's state), which that optimizer's launch advances later in
 * the same update, so a replayed graph draws fresh noise per update and a resumed checkpoint
 * continues the stream.  policy_noise = 0 gives clip(act, low, high).  NaN stays NaN.
 * F110_E_INVALID before any device call for a null required pointer, a bad shape, a negative or
 * non-finite policy_noise / noise_clip, or counter == NULL with normals_ext == NULL. */
F110_API int f110_td3_target_action(const float *h, const float *W, const float *b, const float *scale,
                                    const float *shift, int32_t B, int32_t K, int32_t nout, float policy_noise,
                                    float noise_clip, const float *low, const float *high, uint64_t seed,
                                    const int64_t *counter, const float *normals_ext, float *out, void *stream);
/* f110_ddpg_critic_step for twin critics, in one launch.  Per row, with q1t = ht1 Wt1^T + bt1,
 * q2t = ht2 Wt2^T + bt2 (the two target critics) and q_i = h_i W_i^T + b_i (ht_i, h_i: [B][K]):
 *   m = min(q1t, q2t) (torch.minimum: NaN propagates);  y = r + (gamma (1 - d)) m;  td_i = y - q_i;
 *   dq_i = -((g / B) w) (2 td_i)   (dq1 / dq2: [B], each may be null);
 *   dh_i = dq_i W_i where dh_i_mask > 0   (dh_i may be null; its mask may be null);
 *   td[r] = 0.5 (|td1| + |td2|), the PER priority (non-negative);
 *   part[blk] = block sums of w td1^2 + w td2^2 (f110_ddpg_row_blocks(B) floats; the loss
 *   mean(w td1^2) + mean(w td2^2) is sum(part) / B: f110_learner_wgrad_loss).
 * F110_E_INVALID before any device call for a null required pointer or a bad shape. */
F110_API int f110_td3_critic_step(const float *ht1, const float *Wt1, const float *bt1, const float *ht2,
                                  const float *Wt2, const float *bt2, const float *r, const float *d, float gamma,
                                  const float *h1, const float *W1, const float *b1, const float *h2,
                                  const float *W2, const float *b2, const float *w, const float *g, int32_t B,
                                  int32_t K, float *td, float *dh1, const float *dh1_mask, float *dh2,
                                  const float *dh2_mask, float *dq1, float *dq2, float *part, void *stream);

/* ---- learner GEMMs (fp32 matrix cores) -------------------------------------------
 * The hidden layers of the DDPG networks (agent.py:25-97: fc1 / fc2, fcs1 /
 * fcs2 and replay()'s backward through them, :302-331), forward and backward,
 * as grouped fp32 MFMA launches with the layer's epilogue fused.  Replaces
 * torch.addmm + relu, threshold_backward, torch.cat([z, action]) and the
 * weight / input gradient GEMMs of autograd.  Row-major float32 device
 * buffers; every op of one launch shares M (the batch rows).
 *
 * f110_learner_gemm: for each op,
 *   C[m][n] = epi( sum_k A'[m][k] B(k, n)  +  sum_{t < nx2} x2[m][t] w2[n][t]  +  bias[n] )
 *   A'[m][k] = amask ? (amask[m][k] > 0 ? A[m][k] : 0) : A[m][k]   (amask stride lda)
 *   B(k, n)  = nn ? B[k * ldb + n] : B[n * ldb + k]   (nn = 0: a Linear's weight
 *              [N][K] as in x W^T; nn = 1: the weight itself as in g W)
 *   epi: ReLU when relu != 0 (NaN kept, as torch.relu), then
 *        C := omask[m][n] > 0 ? C : 0 when omask is set (stride ldc).
 * bias, amask, omask, x2 / w2 may be null; nx2 <= 2 (the critic's action
 * columns of fcs2's input, agent.py:94).  All ops of a launch share nn and
 * whether amask is set.
 * Deterministic (fixed summation order); async on stream. */
typedef struct f110_gemm_op {
    const float *A, *B, *bias, *amask, *omask, *x2, *w2;
    float *C;
    int32_t N, K, lda, ldb, ldc, ldx2, ldw2, nx2, relu, nn;
} f110_gemm_op;
F110_API int f110_learner_gemm(const f110_gemm_op *ops, int32_t nops, int32_t M, void *stream);

/* f110_learner_wgrad: a Linear's weight and bias gradients, for each op
 *   dW[n][kx] (stride ldw) = sum_m G'[m][n] X[m][kx],  db[n] = sum_m G'[m][n]
 *   G'[m][n] = gmask ? (gmask[m][n] > 0 ? G[m][n] : 0) : G[m][n]   (gmask stride ldg)
 * (autograd's grad_W = gz^T x and grad_b = gz.sum(0) after threshold_backward).
 * db may be null; all ops of a launch share whether gmask is set.  M is split over blocks; the partial sums go to scratch
 * (f110_learner_wgrad_scratch_floats floats) and are added in a fixed order. */
typedef struct f110_wgrad_op {
    const float *G, *gmask, *X;
    float *dW, *db;
    int32_t N, KX, ldg, ldx, ldw;
} f110_wgrad_op;
F110_API int64_t f110_learner_wgrad_scratch_floats(const f110_wgrad_op *ops, int32_t nops, int32_t M);
F110_API int f110_learner_wgrad(const f110_wgrad_op *ops, int32_t nops, int32_t M, float *scratch, void *stream);
/* f110_learner_wgrad, and in its finishing launch *loss = sign * (sum of loss_part[0 .. n_part), in
 * order) / M: the loss of a fused head (f110_ddpg_critic_step / f110_ddpg_q_mean_step) without a
 * launch of its own. */
F110_API int f110_learner_wgrad_loss(const f110_wgrad_op *ops, int32_t nops, int32_t M, float *scratch,
                                     const float *loss_part, int32_t n_part, float sign, float *loss, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* F110_H */
