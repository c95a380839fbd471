// f110_task_args.h — the argument blocks and launchers of the kernels beside the env step: the
// C-ABI batch kernels, gap-follow, the track, the reward and the pure-pursuit opponent, the episode
// and the race statistics, the track observation, the scan observation, the sensor randomization.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_env_rows.h"
#include "f110_map.h"
#include "f110_race.h"

namespace f110 {

struct ScanArgs {
    MapView map;
    const double *sines, *cosines;
    int32_t B, theta_dis;
    double fov, eps, max_range, inc;
    const double *poses;  // [M][3]
    int64_t M;
    double *scans;        // [M][B]
    int32_t *lookups;     // [M][B] or null
    int32_t *hit_rc;      // [M][B][2] or null
    unsigned long long *ctr;
};

// gap_follow_action over M float32 scans (f110_gap_follow).
struct GapFollowArgs {
    const float *scans;   // scan m at scans + m * scan_stride
    int64_t M, scan_stride, action_stride;
    float *actions;       // (steer, speed) of scan m at actions + m * action_stride
    int32_t *gaps;        // [M][2] chosen (start, end) or null
    double angle_min, angle_increment;
    int32_t B;
};

// CenterlineProgress arrays on the device (f110_track).
struct TrackView {
    const double *xy;   // [n][2]
    const double *s;    // [n] arclength
    const double *tan;  // [n-1][2]
    const double *nrm;  // [n-1][2]
    const double *mid;  // [n-1][2] segment midpoints
    const double *wR, *wL;  // [n] lane widths or null
    int32_t n, closed;
    double L;
    // uniform grid over the midpoints (kd.query acceleration): cell (i, j) of
    // size gh at (gx0 + i*gh, gy0 + j*gh) holds midpoints cell_items[cell_start[c] ..
    // cell_start[c+1]), c = j*gnx + i
    const int32_t *cell_start, *cell_items;
    const double *cell_mid;  // [n-1][2]: mid[cell_items[q]], in cell order (no indirection)
    int32_t gnx, gny;
    double gx0, gy0, gh;
};

struct RewardArgs {
    TrackView track;
    f110_reward_params p;
    const float *obs;
    int64_t E;
    int32_t obs_len, B;
    f110_reward_state *state;
    const uint8_t *reset_mask;
    double *rewards;
};

// f110_pure_pursuit over M cars (k_pursuit, f110_pursuit.hip).
struct PursuitArgs {
    TrackView track;
    f110_pursuit_params p;
    const float *poses;        // (x, y, yaw) of row m at poses + m * pose_stride
    int64_t M, pose_stride, action_stride;
    const double *row_speed;   // [M] or null
    const uint8_t *row_mask;   // [M] or null: rows with 0 keep their bytes
    float *actions;            // (steer, speed) of row m at actions + m * action_stride
    double *aux;               // [M][4] s_proj, t, target x, y, or null
};

// ---- episode statistics (f110_episode.hip) ---------------------------------
constexpr int kEpisodeBlock = 256;  // envs per block of k_episode (the documented reduction order, f110.h)
struct EpisodeArgs {
    const double *rewards;
    const uint8_t *terminated, *truncated, *was_reset;  // truncated may be null
    int64_t E;
    f110_episode_state *state;
    double *last_return;    // the three per-env outputs may be null
    int32_t *last_length;
    uint8_t *finished;
    f110_episode_totals *totals;
    EpisodePart *part;      // [episode_blocks(E)] block partials (the caller's scratch)
};
inline int64_t episode_blocks(int64_t E) { return (E + kEpisodeBlock - 1) / kEpisodeBlock; }
hipError_t launch_episode_stats(const EpisodeArgs &a, hipStream_t s);

// ---- race statistics (f110_race.hip; the row rule: f110_race.h) --------------
constexpr int kRaceBlock = 256;    // envs per block of k_race (the documented reduction order, f110.h)
constexpr int kRaceProjEnvs = 4;   // envs (= waves) per block of k_race_project
struct RaceArgs {
    TrackView track;
    f110_race_params p;
    const float *ego, *opp;  // (x, y, yaw, col) of env e at ego / opp + e * stride; opp may be null
    int64_t stride, E;
    const uint8_t *terminated, *truncated, *was_reset;  // truncated may be null
    f110_race_state *state;
    double *cur;             // [E][2] progress, lead, or null
    double *last_progress, *last_lead;  // the three last_* may be null
    int32_t *last_length;
    uint8_t *result;
    f110_race_totals *totals;
    RaceProj *proj;          // [E] the call's projections (the caller's scratch)
    RacePart *part;          // [race_blocks(E)] block partials (the caller's scratch, after proj)
};
inline int64_t race_blocks(int64_t E) { return (E + kRaceBlock - 1) / kRaceBlock; }
hipError_t launch_race_stats(const RaceArgs &a, hipStream_t s);

// ---- track observation (f110_track_obs.hip; the row rule: f110_track_obs.h) -------------------
struct TrackObsArgs {
    TrackView track;
    f110_track_obs_params p;
    const double *state;  // [7][E*A] f64 (f110_get_state's layout)
    int64_t E, out_stride;
    int32_t A, seat, other, width;  // other: -1 = none; width: f110_track_obs_width
    float *out;           // row e at out + e * out_stride
};
hipError_t launch_track_obs(const TrackObsArgs &a, hipStream_t s);

// ---- scan observation (f110_scan_obs.hip; the row rule: f110_scan_obs.h) ----------------------
struct ScanObsArgs {
    const float *rows;     // row e at rows + e * row_stride: [B | M | T]
    const uint8_t *reset;  // [E] or null
    float *ring;           // [E][D][K]
    int32_t *head;         // [E], -1 = empty
    float *out;            // row e at out + e * out_stride: [F*K | M if keep_mid | T]
    int64_t E, row_stride, out_stride;
    int32_t B, M, T, K, F, S, D, reduce, keep_mid;
    int32_t vec4;          // rows 16-byte aligned and row_stride % 4 == 0: the row is loaded as float4
};
hipError_t launch_scan_obs(const ScanObsArgs &a, hipStream_t s);
hipError_t launch_scan_obs_reset(int32_t *head, const uint8_t *env_mask, int64_t E, hipStream_t s);

// ---- sensor randomization (f110_sensor.hip; the row rule: f110_sensor.h) ----------------------
struct SensorArgs {
    const float *rows;       // row e at rows + e * row_stride: [B | M | T]
    const uint8_t *reset;    // [E] or null
    const uint8_t *mask;     // [E] or null (every env): rows with 0 are copied through
    float *param_rows;       // [E][10] the drawn parameters (SensorRow)
    int32_t *episode;        // [E], -1 = no apply yet
    int32_t *step;           // [E] applies since the episode's start
    float *out;              // row e at out + e * out_stride; may be rows itself
    int64_t E, row_stride, out_stride, env_offset;
    uint64_t seed;
    f110_sensor_params p;
    float range_max;
    int32_t B, M, T;
};
hipError_t launch_sensor(const SensorArgs &a, hipStream_t s);
hipError_t launch_sensor_reset(int32_t *episode, int32_t *step, const uint8_t *env_mask, int64_t E, hipStream_t s);

// ---- the C-ABI batch kernels (f110_batch.hip) and the task kernels ----------------------------
hipError_t launch_scan_batch(const ScanArgs &a, hipStream_t s);
hipError_t launch_gap_follow(const GapFollowArgs &a, hipStream_t s);
hipError_t launch_reward(const RewardArgs &a, hipStream_t s);
hipError_t launch_pursuit(const PursuitArgs &a, hipStream_t s);
size_t gap_follow_lds_bytes(int B);
hipError_t launch_dynamics_ks_batch(const double *x, const double *u, double *f, int64_t M, const f110_params &p,
                                    hipStream_t s);
hipError_t launch_collision_batch(const double *v1, const double *v2, int64_t M, uint8_t *out, hipStream_t s);
hipError_t launch_collision_multiple(const double *verts, int64_t M, int32_t N, double *collisions, double *idx,
                                     hipStream_t s);
hipError_t launch_dynamics_batch(const double *x, const double *u, double *f, int64_t M, const f110_params &p,
                                 hipStream_t s);

}  // namespace f110
