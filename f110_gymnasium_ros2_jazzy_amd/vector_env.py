"""F110VectorEnv: N F1TENTH envs stepped as one batch on one GPU.

Gymnasium-1.x vector surface (``reset(seed, options) -> (obs, infos)``,
``step(actions) -> (obs, rewards, terminations, truncations, infos)``,
``num_envs``, ``single_observation_space``, ``single_action_space``) with
observations and infos kept as device tensors (``as_numpy=True`` converts).

Per env the semantics are F110Env's (f110_env.py:371-472): reward = timestep,
terminated = ego collision or 4 lap toggles, truncated = False (unless episode
limits are set, below), flat obs =
[agent-0 scan / lidar_max, (x, y, yaw, collision) per agent].  Autoreset is
the gymnasium NEXT_STEP mode and runs on the device: the step after an env
terminates resets it to a pose drawn from ``spawn_poses`` (and performs the
reference's zero-action reset step); that step's reward is 0.

``reward_fn`` (a reward.BatchedCenterlineReward) replaces the timestep
reward with the training reward train_ddpg.py computes per step, evaluated on
the device; autoreset steps reset its state and are rewarded 0.

``opponent="gap_follow"`` drives agent ``opponent_idx`` with the reference's
rule-based opponent (gap_follow.py) on the device, as train_ddpg.py:168 does
on the host: its action for step t comes from its own float32 scan of step
t-1 (or of the reset).  ``step`` then takes the other agents' actions
([N, 2] for two agents) and ``infos["opponent_actions"]`` shows the
opponent's.  ``opponent="policy"`` drives it with ``opponent_policy`` (an
opponent.PolicyOpponent: a frozen Actor's noise-free action from the
opponent's own seat, same timing), ``opponent="mixed"`` with the policy in the
envs where ``opponent_mask`` (uint8 [N]) is set and gap_follow in the others;
the infos and the action rows are the same for all three.
``opponent="pure_pursuit"`` drives it with the waypoint follower of opponent.pure_pursuit on
``opponent_track`` (a device reward.CenterlineTrack): its action for step t comes from its pose in
step t-1's observation (same timing), with ``opponent_params`` (lookahead, speed, ... see
opponent.pursuit_params) and, for a population of opponents, ``opponent_speed`` (one speed for
all, or one per env).  ``opponent="mixed"`` takes ``opponent_rule="gap_follow" | "pure_pursuit"``
for the envs the policy does not drive.

``param_ranges`` ({field: (lo, hi)}, or one such dict per agent) turns on the
device's domain randomization of the vehicle dynamics: every reset and
autoreset redraws the resetting cars' friction, mass, ... from the ranges
(keyed by global env id and episode); ``env.sim.env_params()`` shows the cars
in force.  The infos are unchanged.

``spawn_ranges`` ({"lateral": (lo, hi), "heading": (lo, hi), "speed": (lo, hi), "gap": (lo, hi),
"behind": p, "clearance": c}, or one such dict per agent) turns on the device's start-state
randomization (BatchSim.set_spawn_randomization), keyed by ``spawn_seed``: every reset and autoreset
starts the resetting cars off the base pose, turned and rolling, and in autoresets an agent with a
``gap`` that many spawn rows ahead of or behind the env's row; ``env.sim.spawn_state()`` shows the
drawn starts.  The infos are unchanged.

``max_episode_steps`` / ``stall_speed`` + ``stall_steps`` put episode limits on
the device (BatchSim.set_episode_limits): an env that did not terminate is
truncated after ``max_episode_steps`` steps since its reset (code 1), or when
its ego has been slower than ``stall_speed`` for ``stall_steps`` steps in a row
(code 2); terminated wins over the time limit, the time limit over the stall.
``step`` then returns the device's truncations, ``infos["truncation"]`` holds
the u8 code, and a truncated env autoresets at its next step exactly as a
terminated one does.  A trainer stores a truncated transition with ``done`` =
0 (DDPGLearner.remember_env takes ``terminated``): it bootstraps from its real
next_obs, which under NEXT_STEP autoreset is what the truncating step returns;
the reset row that follows is skipped as after a termination.  With all limits
off (the default) truncations stay zeros and the infos keys are unchanged.

``episode_stats=True`` keeps per-env episode returns and lengths on the device
(episode.EpisodeStats, one small kernel pair per step on that step's rewards):
``infos["episode"]`` = {"r": last finished return, "l": its length, "finished":
the envs that finished in this step}, ``episode_totals()`` the running totals.

``race_stats=True`` keeps per-env race outcomes on the device (race.RaceStats, three small launches
per step on the obs buffer the reward sees): ``infos["race"]`` = {"progress": the running episode's
centerline progress of the ego in m, "lead": its lead over the opponent, "result": the result byte
of the envs that finished in this step (include/f110.h, "race statistics"), "finished": its bit 0},
``race_totals()`` the running totals (progress, lead, passes, crashes, win rate).  The centerline is
``race_track`` (a device reward.CenterlineTrack), by default ``reward_fn.progress``, then
``opponent_track``; the opponent is agent ``opponent_idx`` when ``num_agents >= 2``; ``race_params``
= {"pass_margin", "direction"}.  Off (the default) the infos keys are unchanged.

``track_obs=True`` (or a dict of track_obs.track_obs_params names) appends the track-relative block
of track_obs.TrackObs to every observation: the ego's speed, steering angle, yaw rate and slip, its
lateral offset and heading error on the centerline, a preview of the centerline ahead in its own
frame and, with ``num_agents >= 2``, the gap to agent ``opponent_idx``.  Observations are then
``[N, B + 4A + width]``: the env owns the wide buffer, the simulator writes its left ``B + 4A``
columns in place (the rows' stride is the wide width) and one more launch per step fills the tail
from the simulator's live state.  The centerline is ``obs_track`` (a device
reward.CenterlineTrack), by default ``reward_fn.progress``, then ``opponent_track``, then
``race_track``.  The reward, the race statistics and the opponents read the wide rows; the infos are
unchanged.  Off (the default) nothing differs.

``scan_obs=True`` (or a dict of scan_obs.scan_obs_params names: n_bins, n_frames, stride, reduce,
keep_mid) makes the observation compact on the device (scan_obs.ScanObs): the ``B`` range columns
pooled into ``n_bins`` sectors, the last ``n_frames`` pooled frames stacked ``stride`` steps apart,
newest first, the pose groups carried through (or dropped: ``keep_mid=False``) and the track block,
if any, after them.  The env owns the full-width buffer, the simulator writes its left columns and
every existing stage (the track observation's fill, the opponents, the reward, the statistics) reads
it unchanged; one more launch then makes the compact rows ``step``, ``reset`` and
``step_transition`` return (``obs_out`` is then a compact buffer), which ``obs_dim`` and
``single_observation_space`` describe.  ``full_obs`` is the last full rows, valid until the next
step.  ``reset()`` empties the ring; a ``was_reset`` row (a NEXT_STEP autoreset: the new episode's
first frame) refills its ring, so all of its stacked frames are that frame.  Off (the default)
nothing differs.

``sensor_ranges`` ({"scale" | "noise_abs" | "noise_rel" | "dropout" | "blackout" | "quant" | "pose_xy" |
"pose_theta": (lo, hi)}, see sensor.sensor_ranges) turns on the device's sensor randomization
(sensor.SensorModel), keyed by ``sensor_seed`` and the global env id: every reset and autoreset
redraws the env's sensor parameters, and one more launch per step and reset turns the full rows
into the rows ``step``, ``reset`` and ``step_transition`` return -- the ranges scaled, noised,
quantized, dropped and blacked out, the pose columns noised.  The stage runs after the opponents,
the reward and the statistics have read the clean rows (``full_obs`` stays clean) and before the
scan observation, which then pools the corrupted rows.  ``sensor_mask`` (uint8 [N]): the envs the
stage touches; an env with 0 gets its clean row (a trainer's evaluation envs).
``sensor_params()`` shows the drawn rows.  A self-play snapshot (PolicyOpponent) keeps seeing clean
rows from its own seat.  Off (the default) nothing differs.

Multi-GPU: give each rank its block of envs (distributed.shard_range) and
``env_offset`` = the block's first global id; RNG streams are keyed by global
env id, so results do not depend on the GPU count.
"""
from __future__ import annotations

import numpy as np
import torch

from ._dev import device_track, f32_rows, first_track
from .f110_env import DEFAULT_PARAMS, _box
from .maps import centerline_spawns, load_map
from .sim import BatchSim, param_range_rows, spawn_range_rows


class F110VectorEnv:
    metadata = {"autoreset_mode": "NextStep", "render_modes": []}

    def __init__(self, num_envs: int, map: str = "Spielberg_map", map_ext: str = ".png", num_agents: int = 1,
                 params: dict | None = None, seed: int = 42, timestep: float = 0.01, device=0,
                 spawn_poses: np.ndarray | None = None, noise_std: float = 0.01, env_offset: int = 0,
                 ego_idx: int = 0, as_numpy: bool = False, autoreset: bool = True, opponent: str | None = None,
                 opponent_idx: int = 1, reward_fn=None, infos: str = "full", options_dtype=np.float32,
                 param_ranges=None, param_seed: int | None = None, max_episode_steps: int | None = None,
                 stall_speed: float = 0.0, stall_steps: int | None = None, episode_stats: bool = False,
                 opponent_policy=None, opponent_mask=None, opponent_track=None, opponent_params: dict | None = None,
                 opponent_speed=None, opponent_rule: str = "gap_follow", race_stats: bool = False, race_track=None,
                 race_params: dict | None = None, track_obs=None, obs_track=None, scan_obs=None, spawn_ranges=None,
                 spawn_seed: int | None = None, sensor_ranges=None, sensor_seed: int | None = None, sensor_mask=None,
                 **kwargs):
        self.num_envs = int(num_envs)
        self.num_agents = int(num_agents)
        self.params = dict(params or DEFAULT_PARAMS)
        # a bad sensor range or mask: ValueError before anything is built
        sens_params = self._check_sensor(sensor_ranges, sensor_seed, sensor_mask, int(kwargs.get("num_beams", 1080)),
                                         env_offset)
        # a bad scan-observation parameter: ValueError before anything is built
        sobs_params = self._check_scan_obs(scan_obs, int(kwargs.get("num_beams", 1080)))
        # a bad opponent argument: ValueError before anything is built
        self._check_opponent(opponent, int(opponent_idx), opponent_policy, opponent_mask, opponent_track,
                             opponent_params, opponent_speed, opponent_rule, device)
        if param_ranges is not None:  # an unknown field: ValueError before anything is built
            param_range_rows(param_ranges, [{**DEFAULT_PARAMS, **self.params}] * self.num_agents)
        if spawn_ranges is not None:  # an unknown name, a value that is no pair: ValueError before anything is built
            spawn_range_rows(spawn_ranges, self.num_agents)
        # a track observation without a usable centerline: ValueError before anything is built
        obs_track, tobs_params = self._check_track_obs(track_obs, obs_track, reward_fn, opponent_track, race_track,
                                                       device, int(ego_idx), int(opponent_idx))
        # race statistics without a usable centerline: ValueError before anything is built
        race_track = self._check_race(race_stats, race_track, race_params, reward_fn, opponent_track, device,
                                      int(ego_idx), int(opponent_idx))
        # a bad episode limit: ValueError before anything is built
        limits = BatchSim.check_episode_limits(max_episode_steps, stall_speed, stall_steps)
        self.timestep = timestep
        self.as_numpy = as_numpy
        self.track = load_map(map, map_ext)
        if spawn_poses is None:
            spawn_poses = centerline_spawns(map.replace("_map", ""), self.num_agents)
        self.spawn_poses = np.ascontiguousarray(spawn_poses, dtype=np.float64)
        self.sim = BatchSim(self.track, n_envs=self.num_envs, n_agents=self.num_agents, params=self.params,
                            device=device, seed=seed, timestep=timestep, ego_idx=ego_idx, noise_std=noise_std,
                            autoreset=autoreset, spawn_poses=self.spawn_poses, env_offset=env_offset, **kwargs)
        self.device = self.sim.device
        # domain randomization (BatchSim.set_param_randomization), on before the first reset: every
        # reset and device autoreset redraws the resetting cars' dynamics; sim.env_params() shows them
        if param_ranges is not None:
            self.sim.set_param_randomization(param_ranges, seed=param_seed)
        # start-state randomization (BatchSim.set_spawn_randomization), on before the first reset
        if spawn_ranges is not None:
            self.sim.set_spawn_randomization(spawn_ranges, seed=spawn_seed)
        # episode limits on the device (BatchSim.set_episode_limits), on before the first reset
        self._limits = bool(limits[0] or limits[2])
        if self._limits:
            self.sim.set_episode_limits(max_episode_steps, stall_speed, stall_steps)
        self._episode = None
        if episode_stats:
            from .episode import EpisodeStats
            self._episode = EpisodeStats(self.num_envs, device=self.device)
        self._race = None
        if race_stats:
            from .race import RaceStats
            self._race = RaceStats(self.num_envs, race_track, self.sim.B, ego_idx=ego_idx,
                                   opponent_idx=int(opponent_idx) if self.num_agents >= 2 else None,
                                   device=self.device, **(race_params or {}))
        # F110Env.reset computes start_rot in the dtype of its options
        # (f110_env.py:448-451): autoresets and option-less resets follow
        # options_dtype (train_ddpg passes float32 poses); an explicit
        # reset(options=...) follows that array's dtype
        self.options_dtype = np.dtype(options_dtype)
        self.sim.set_reset_dtype(self.options_dtype)
        B, A = self.sim.B, self.num_agents
        x_min, x_max, y_min, y_max = self.track.bounds
        obs_low = np.array([0.0] * B + [x_min, y_min, -np.pi, 0.0] * A, np.float32)
        obs_high = np.array([1.0] * B + [x_max, y_max, np.pi, 1.0] * A, np.float32)
        # the track observation: the env's own wide buffer, whose left B + 4A columns the simulator
        # writes in place and whose tail TrackObs.fill writes after every step and reset
        self._tobs = self._wide = None
        if obs_track is not None:
            from .track_obs import TrackObs
            self._tobs = TrackObs(self.sim, obs_track, seat=int(ego_idx),
                                  other=int(opponent_idx) if A >= 2 else None, **tobs_params)
            self._head = B + 4 * A
            self._wide = torch.zeros(self.num_envs, self._head + self._tobs.width, dtype=torch.float32,
                                     device=self.device)
            obs_low, obs_high = np.concatenate([obs_low, self._tobs.low]), np.concatenate([obs_high, self._tobs.high])
        # the sensor randomization: every stage keeps reading the clean full rows in the env's own
        # buffer (the one above, or one of B + 4A columns); one more launch per step and reset makes
        # the rows seen through the sensor, in a buffer of its own or, when nothing follows, obs_out
        self._sensor = self._noisy = None
        if sens_params is not None:
            from .sensor import SensorModel
            self._head = B + 4 * A
            if self._wide is None:
                self._wide = torch.zeros(self.num_envs, self._head, dtype=torch.float32, device=self.device)
            lidar_max = float({**DEFAULT_PARAMS, **self.params}["lidar_max"])
            self._sensor = SensorModel(self.num_envs, B, 4 * A, self._wide.shape[1] - self._head, range_max=lidar_max,
                                       seed=int(self.sim.cfg.seed) if sensor_seed is None else int(sensor_seed),
                                       env_offset=env_offset, mask=sensor_mask, device=self.device, **sens_params)
            self._noisy = torch.zeros_like(self._wide)
        # the scan observation: every stage keeps reading the full rows in the env's own buffer (the
        # one above, or one of B + 4A columns); one more launch per step and reset makes the compact
        # rows the caller gets back
        self._sobs = self._compact = self._last_full = None
        if sobs_params is not None:
            from .scan_obs import ScanObs, scan_obs_columns
            self._head = B + 4 * A
            if self._wide is None:
                self._wide = torch.zeros(self.num_envs, self._head, dtype=torch.float32, device=self.device)
            tail = self._wide.shape[1] - self._head
            self._sobs = ScanObs(self.num_envs, B, 4 * A, tail, device=self.device, **sobs_params)
            self._compact = torch.zeros(self.num_envs, self._sobs.width, dtype=torch.float32, device=self.device)
            obs_low, obs_high = scan_obs_columns(self._sobs.params, obs_low[B:self._head], obs_high[B:self._head],
                                                 obs_low[self._head:], obs_high[self._head:])
        self.obs_dim = int(obs_low.shape[0])
        self.single_observation_space = _box(obs_low, obs_high)
        low = np.array([self.params["s_min"], self.params["v_min"]], np.float32)
        high = np.array([self.params["s_max"], self.params["v_max"]], np.float32)
        self.single_action_space = _box(np.tile(low, (A, 1)), np.tile(high, (A, 1)))
        self._rng = np.random.default_rng(seed)
        self.opponent = opponent
        self.opponent_idx = int(opponent_idx)
        # reward_fn: a BatchedCenterlineReward (reward.py) evaluated on the device
        # from every step's observations, as train_ddpg.py:176 does per env
        self.reward_fn = reward_fn
        # infos="minimal": only "reset" (+ "opponent_actions"), no per-step copies
        # of the scans and poses (the batched trainer reads nothing else)
        if infos not in ("full", "minimal"):
            raise ValueError("infos must be 'full' or 'minimal'")
        self.infos_mode = infos
        if reward_fn is not None and reward_fn.n_envs != self.num_envs:
            raise ValueError("reward_fn must be built for num_envs envs")
        self.opponent_policy = opponent_policy if opponent in ("policy", "mixed") else None
        self.opponent_mask = None
        if self.opponent_policy is not None and (self.opponent_policy.obs_dim != self.obs_dim
                                                 or self.opponent_policy.device != self.device):
            raise ValueError(f"opponent_policy must take {self.obs_dim} observations on {self.device}")
        # the rule opponent: of every env ("gap_follow", "pure_pursuit"), of the unmasked ones ("mixed")
        self.opponent_rule = {None: None, "policy": None, "mixed": opponent_rule}.get(opponent, opponent)
        self.opponent_track = self._pursuit_params = self._pursuit_speed = None
        if self.opponent_rule == "pure_pursuit":
            self.opponent_track = opponent_track
            self._pursuit_params = dict(opponent_params or {})
            if opponent_speed is not None:
                sp = np.broadcast_to(np.asarray(opponent_speed, dtype=np.float64), (self.num_envs,))
                self._pursuit_speed = torch.as_tensor(np.array(sp), device=self.device)  # (a writable copy)
        if opponent is not None:
            if opponent == "mixed":
                m = torch.as_tensor(opponent_mask)
                m = m.view(torch.uint8) if m.dtype == torch.bool else m
                self.opponent_mask = m.to(self.device).contiguous()
            self._act = torch.zeros(self.num_envs, A, 2, dtype=torch.float32, device=self.device)
            self._others = [i for i in range(A) if i != self.opponent_idx]
            # a contiguous run of caller-driven agents is written with a slice
            # copy (one strided copy kernel) instead of an index_put
            o = self._others
            self._others_sl = slice(o[0], o[-1] + 1) if o and o == list(range(o[0], o[-1] + 1)) else o

    OPPONENTS = ("gap_follow", "policy", "mixed", "pure_pursuit")
    RULES = ("gap_follow", "pure_pursuit")

    def _check_opponent(self, opponent, idx, policy, mask, track=None, params=None, speed=None, rule="gap_follow",
                        device=0):
        """The opponent arguments against each other and the env's shape (host values only)."""
        if opponent is None:
            return
        N, A = self.num_envs, self.num_agents
        if opponent not in self.OPPONENTS:
            raise ValueError(f"unknown opponent policy {opponent!r} (supported: 'gap_follow', 'policy', 'mixed', "
                             "'pure_pursuit')")
        if not (0 <= idx < A) or A < 2:
            raise ValueError("opponent needs num_agents >= 2 and 0 <= opponent_idx < num_agents")
        if opponent == "mixed" and rule not in self.RULES:
            raise ValueError(f"unknown opponent_rule {rule!r} (supported: 'gap_follow', 'pure_pursuit')")
        if opponent == "pure_pursuit" or (opponent == "mixed" and rule == "pure_pursuit"):
            self._check_pursuit(track, params, speed, device)
        if opponent in self.RULES:
            return
        if policy is None:
            raise ValueError(f"opponent={opponent!r} needs opponent_policy (an opponent.PolicyOpponent)")
        lidar_max = float({**DEFAULT_PARAMS, **self.params}["lidar_max"])
        if policy.n_envs != N or policy.act_dim != 2 or policy.lidar_max != lidar_max:
            raise ValueError(f"opponent_policy must be built for {N} envs, 2 action columns and lidar_max {lidar_max}")
        if opponent == "mixed":
            if mask is None:
                raise ValueError("opponent='mixed' needs opponent_mask (uint8 [num_envs])")
            if tuple(mask.shape) != (N,) or str(mask.dtype).split(".")[-1] not in ("uint8", "bool"):
                raise ValueError(f"opponent_mask must be a uint8 [{N}] array or tensor")

    def _check_pursuit(self, track, params, speed, device):
        """The pure-pursuit arguments: a device track on the env's device, known parameter names,
        one speed or one per env (host values only)."""
        from .opponent import PURSUIT_FIELDS, check_pursuit_speed
        device_track(track, device, "opponent_track",
                     "opponent 'pure_pursuit' needs opponent_track (a device reward.CenterlineTrack)")
        unknown = sorted(set(params or {}) - set(PURSUIT_FIELDS))
        if unknown:
            raise ValueError(f"unknown opponent_params {unknown} (known: {', '.join(PURSUIT_FIELDS)})")
        check_pursuit_speed(speed, self.num_envs)

    def _check_track_obs(self, track_obs, track, reward_fn, opponent_track, race_track, device, ego_idx, opponent_idx):
        """The track-observation arguments (host values only): (the centerline to use, the parameter
        dict), or (None, None) when off."""
        if track_obs is None or track_obs is False:
            return None, None
        from .track_obs import MAX_PREVIEW, TRACK_OBS_FIELDS
        if track_obs is not True and not isinstance(track_obs, dict):
            raise ValueError("track_obs must be None, True or a dict of track-observation parameters")
        params = {} if track_obs is True else dict(track_obs)
        unknown = sorted(set(params) - set(TRACK_OBS_FIELDS))
        if unknown:
            raise ValueError(f"unknown track_obs parameters {unknown} (known: {', '.join(TRACK_OBS_FIELDS)})")
        track = device_track(first_track(track, getattr(reward_fn, "progress", None), opponent_track, race_track),
                             device, "the track observation's centerline",
                             "track_obs needs a centerline: obs_track, reward_fn.progress, opponent_track or "
                             "race_track (a device reward.CenterlineTrack)")
        if params.get("direction", 1) not in (1, -1):
            raise ValueError("track_obs: direction must be +1 or -1")
        prev = [float(d) for d in params.get("preview", ())]
        if len(prev) > MAX_PREVIEW or any(not 0.0 < d < track.L for d in prev):
            raise ValueError(f"track_obs: preview takes at most {MAX_PREVIEW} distances in (0, {track.L}) m")
        for k in set(params) - {"direction", "preview"}:
            if not float(params[k]) > 0.0:
                raise ValueError(f"track_obs: {k} must be > 0; got {params[k]!r}")
        if not 0 <= ego_idx < self.num_agents:
            raise ValueError("track_obs: ego_idx must be an agent")
        if self.num_agents >= 2 and (opponent_idx == ego_idx or not 0 <= opponent_idx < self.num_agents):
            raise ValueError("track_obs: opponent_idx must be another agent than ego_idx")
        return track, params

    @staticmethod
    def _check_scan_obs(scan_obs, n_beams):
        """The scan-observation argument (host values only): the parameter dict, or None when off."""
        if scan_obs is None or scan_obs is False:
            return None
        if scan_obs is not True and not isinstance(scan_obs, dict):
            raise ValueError("scan_obs must be None, True or a dict of scan-observation parameters")
        from .scan_obs import scan_obs_params
        params = {} if scan_obs is True else dict(scan_obs)
        scan_obs_params(n_beams, **params)  # unknown names, values out of range: ValueError
        return params

    def _check_sensor(self, ranges, seed, mask, n_beams, env_offset):
        """The sensor-randomization arguments (host values only): the range dict, or None when off."""
        if ranges is None:
            if seed is not None or mask is not None:
                raise ValueError("sensor_seed and sensor_mask need sensor_ranges")
            return None
        if not isinstance(ranges, dict):
            raise ValueError("sensor_ranges must be None or a dict {name: (lo, hi)} of sensor.sensor_ranges names")
        from .sensor import _mask, sensor_ranges
        if not 1 <= n_beams <= 4096:
            raise ValueError(f"sensor_ranges: num_beams must be in [1, 4096]; got {n_beams}")
        sensor_ranges(n_beams, **ranges)  # unknown names, values out of range: ValueError
        _mask(mask, self.num_envs)
        if int(env_offset) < 0:
            raise ValueError("sensor_ranges: env_offset must be >= 0")
        return dict(ranges)

    def sensor_params(self):
        """The sensor parameters in force, as sim.env_params() shows the cars: float32 [N, 10] on the
        device, one row per env (sensor.PARAM_ROW names the columns).  ValueError with the stage off."""
        if self._sensor is None:
            raise ValueError("sensor_params: build the env with sensor_ranges")
        return self._sensor.arrays()["params"]

    def _check_race(self, race_stats, track, params, reward_fn, opponent_track, device, ego_idx, opponent_idx):
        """The race-statistics arguments (host values only): the centerline to use, or None when off."""
        if not race_stats:
            return None
        track = device_track(first_track(track, getattr(reward_fn, "progress", None), opponent_track), device,
                             "the race track", "race_stats=True needs a centerline: race_track, reward_fn.progress "
                             "or opponent_track (a device reward.CenterlineTrack)")
        unknown = sorted(set(params or {}) - {"pass_margin", "direction"})
        if unknown:
            raise ValueError(f"unknown race_params {unknown} (known: pass_margin, direction)")
        pm, d = (params or {}).get("pass_margin"), (params or {}).get("direction", 1)
        if (pm is not None and not float(pm) >= 0.0) or d not in (1, -1):
            raise ValueError("race_params: pass_margin must be >= 0 and direction +1 or -1")
        if self.num_agents >= 2 and (opponent_idx == ego_idx or not 0 <= opponent_idx < self.num_agents):
            raise ValueError("race_stats: opponent_idx must be another agent than ego_idx")
        return track

    def _opponent_next(self, out, obs=None):
        """Next step's opponent action from this step's outputs: gap_follow from its scan
        (train_ddpg.py:168); "policy": the PolicyOpponent's forward from the opponent's seat (obs: the
        step's obs when the simulator wrote it elsewhere than out.obs); "mixed": gap_follow writes
        every row, then the policy head overwrites the rows with opponent_mask != 0 -- the policy's
        hidden layers still run over all N rows (one fixed-shape GEMM pair, whatever the mask).
        "pure_pursuit" (alone, or as the rule of "mixed"): the waypoint follower on the opponent's
        pose group of the step's obs."""
        if self.opponent is None:
            return
        rows = self._act[:, self.opponent_idx]
        if self.opponent_rule == "gap_follow":
            from .opponent import gap_follow
            gap_follow(out.scans[:, self.opponent_idx], out=rows)
        elif self.opponent_rule == "pure_pursuit":
            from .opponent import pure_pursuit
            o = out.obs if obs is None else obs
            g = self.sim.B + 4 * self.opponent_idx  # the obs row's pose groups are in agent order
            pure_pursuit(o[:, g:g + 3], self.opponent_track, out=rows, row_speed=self._pursuit_speed,
                         **self._pursuit_params)
        if self.opponent_policy is not None:
            self.opponent_policy.act(out, self.opponent_idx, rows, row_mask=self.opponent_mask, obs=obs)

    # ------------------------------------------------------------------
    def _episode_infos(self, infos, out):
        """The keys the episode limits / statistics add (none with both off)."""
        if self._limits:
            infos["truncation"] = out.truncated.clone()
        if self._episode is not None:
            ep = self._episode
            infos["episode"] = {"r": ep.last_return.clone(), "l": ep.last_length.clone(),
                                "finished": ep.finished.bool()}
        if self._race is not None:
            rc = self._race
            infos["race"] = {"progress": rc.progress.clone(), "lead": rc.lead.clone(), "result": rc.result.clone(),
                             "finished": rc.finished}
        return infos

    def _to_numpy(self, infos):
        return {k: self._to_numpy(v) if isinstance(v, dict) else v.cpu().numpy() for k, v in infos.items()}

    def _infos(self, out):
        if self.infos_mode == "minimal":
            infos = {"reset": out.was_reset.bool()}
            if self.opponent is not None:
                infos["opponent_actions"] = self._act[:, self.opponent_idx]
            infos = self._episode_infos(infos, out)
            return self._to_numpy(infos) if self.as_numpy else infos
        st = self.sim.agent_states()  # [E, A, 7]
        infos = {
            "poses_x": st[..., 0].float(), "poses_y": st[..., 1].float(), "poses_theta": st[..., 4].float(),
            "linear_vels_x": st[..., 3].float(), "ang_vels_z": st[..., 5].float(),
            "collisions": out.collisions.to(torch.int8), "lap_times": out.lap_times.clone(),
            "lap_counts": out.lap_counts.clone(), "scans": out.scans.clone(), "time": out.sim_time.clone(),
            "reset": out.was_reset.bool(),
        }
        if self.opponent is not None:
            infos["opponent_actions"] = self._act[:, self.opponent_idx].clone()
        infos = self._episode_infos(infos, out)
        if self.as_numpy:
            infos = self._to_numpy(infos)
        return infos

    def reset(self, seed=None, options=None):
        """options: poses [N, A, 3] (or [A, 3] for every env); default: spawn table draws."""
        if seed is not None:
            self._rng = np.random.default_rng(seed)
        if options is None:
            idx = self._rng.integers(0, self.spawn_poses.shape[0], self.num_envs)
            options = self.spawn_poses[idx].astype(self.options_dtype)
        dt = options.dtype if hasattr(options, "dtype") else np.asarray(options).dtype
        self.sim.set_reset_dtype(dt)
        out = self.sim.reset(options)
        self.sim.set_reset_dtype(self.options_dtype)  # the device autoresets
        src = out.obs if self._wide is None else self._fill_wide(out.obs)
        self._last_full = src
        scan_opp = getattr(self.opponent_policy, "scan_obs", None)
        if scan_opp is not None:  # the snapshot's own ring starts over with the env
            scan_opp.reset()
        self._opponent_next(out, None if self._wide is None else src)
        if self.reward_fn is not None:
            self.reward_fn.reset()
        if self._episode is not None:
            self._episode.reset()
        if self._race is not None:
            self._race.reset()
            self._race.begin(src)
        if self._sensor is not None:  # the counters start over: episode 0 of every env, its parameters redrawn
            self._sensor.reset()
            src = self._sensor.apply(src, out=self._noisy)
        if self._sobs is not None:  # an empty ring: every stacked frame is the reset's
            self._sobs.reset()
            src = self._sobs.push(src, out=self._compact)
        obs = src.clone()
        return (obs.cpu().numpy() if self.as_numpy else obs), self._infos(out)

    def _fill_wide(self, head=None, wide=None):
        """The full observation rows in the env's own buffer (track_obs or scan_obs on): the
        simulator's ``head`` columns copied in if given (a reset; a step writes them in place), then
        the track observation's tail, if any."""
        wide = self._wide if wide is None else wide
        if head is not None:
            wide[:, :self._head] = head
        if self._tobs is not None:
            self._tobs.fill(wide[:, self._head:])
        return wide

    @property
    def full_obs(self):
        """The last full observation rows [N, B + 4A (+ the track block)] every stage read (the reward,
        the statistics, the opponents): with scan_obs on what the compact rows were made from.
        Read-only, valid until the next step or reset; None before the first reset."""
        return self._last_full

    def _route(self, actions, own_rows=False):
        """The step's [N, A, 2] action rows: with an opponent the caller's rows copied into the env's
        action buffer beside the opponent's (own_rows: unless they are agent_actions() itself), else
        the caller's tensor."""
        a = torch.as_tensor(actions, device=self.device)
        if self.opponent is None:
            return a.unsqueeze(1) if a.dim() == 2 and self.num_agents == 1 else a
        dst = self.agent_actions() if own_rows else None
        if dst is None or a.data_ptr() != dst.data_ptr() or a.stride() != dst.stride():
            if own_rows or a.dim() == 2:
                a = a.reshape(self.num_envs, len(self._others), 2)
            if not own_rows and a.shape[1] == self.num_agents:  # every agent's rows: the opponent's are dropped
                a = a[:, self._others_sl]
            self._act[:, self._others_sl] = a
        return self._act

    def _advance(self, a, obs_out=None):
        """One step of every stage, in order: the simulator (into obs_out, if given), the track
        observation's tail, the next opponent action, the reward, the episode and race statistics,
        the sensor randomization's rows, the scan observation's compact rows.  Returns (out, obs,
        rewards): the simulator's outputs, the rows the caller gets (what every stage read: the
        simulator's own, the env's wide buffer, or obs_out; with sensor_ranges on those rows seen
        through the sensor, in the stage's own buffer or obs_out; with scan_obs on the compact rows
        made from them, in the env's compact buffer or obs_out) and the reward's own buffer."""
        if self._wide is None:
            out = self.sim.step(a, obs_out=obs_out)  # the simulator writes obs_out itself (no copy)
            obs = out.obs if obs_out is None else obs_out
        else:  # the simulator writes the left columns of the wide rows, one launch fills the tail
            obs = self._wide
            if obs_out is not None:  # (checked before the simulator moves)
                obs_out = f32_rows(obs_out, self.num_envs, self.obs_dim, self.device, "obs_out", copy_ok=False)[0]
                if self._sobs is None and self._sensor is None:
                    obs = obs_out
            out = self.sim.step(a, obs_out=obs[:, :self._head])
            self._fill_wide(wide=obs)
        self._last_full = obs
        self._opponent_next(out, None if obs is out.obs else obs)
        if self.reward_fn is not None:  # reset envs: reward_fn.reset(), reward 0 (the u8 flags as they are)
            rewards = self.reward_fn(obs, reset_mask=out.was_reset)
        else:
            rewards = torch.where(out.was_reset.bool(), torch.zeros((), dtype=torch.float64, device=self.device),
                                  torch.full((), self.timestep, dtype=torch.float64, device=self.device))
        if self._episode is not None:
            self._episode.update(rewards, out.terminated, out.truncated, out.was_reset)
        if self._race is not None:
            self._race.update(obs, out.terminated, out.truncated, out.was_reset)
        if self._sensor is not None:  # the rows seen through the sensor; a reset row starts its env's next episode
            last = self._sobs is None and obs_out is not None  # nothing follows: straight into obs_out
            obs = self._sensor.apply(obs, reset=out.was_reset, out=obs_out if last else self._noisy)
        if self._sobs is not None:  # the compact rows of the full ones; a reset row refills its ring
            obs = self._sobs.push(obs, reset=out.was_reset, out=self._compact if obs_out is None else obs_out)
        return out, obs, rewards

    def step(self, actions):
        out, src, rewards = self._advance(self._route(actions))
        if self.reward_fn is not None:
            rewards = rewards.clone()
        term = out.terminated.bool()
        trunc = out.truncated.bool() if self._limits else torch.zeros_like(term)
        obs = src.clone()
        if self.as_numpy:
            return (obs.cpu().numpy(), rewards.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                    self._infos(out))
        return obs, rewards, term, trunc, self._infos(out)

    def agent_actions(self):
        """The learning agent's rows of the action buffer the next step reads
        ([N, 2] view), or None (no opponent, or several learning agents): a
        policy may write its actions here (DDPGLearner.choose_action(out=...))
        and pass the same view to step_transition(), which then copies nothing."""
        if self.opponent is None or len(self._others) != 1:
            return None
        return self._act[:, self._others[0]]

    def step_transition(self, actions, obs_out=None):
        """step() for a trainer on the device: (next_obs copy [N, obs_dim],
        rewards float64 [N], terminated uint8 [N], was_reset uint8 [N]).  The
        rewards and flags are the simulator's / reward function's own buffers
        (no clone, no dtype conversion): valid until the next step.  obs_out:
        a preallocated [N, obs_dim] float32 tensor to copy next_obs into (a
        captured step graph's fixed buffer) instead of a new one.
        With episode limits on, ``self.truncated`` is this step's u8 flag buffer
        (valid until the next step); the 4-tuple is unchanged, and a trainer keeps
        storing ``terminated`` as done: a truncated transition bootstraps from its
        next_obs, and the reset row after it is skipped like any other.
        With track_obs on obs_dim is the wide width and obs_out a wide buffer, whose tail is filled too.
        With scan_obs on obs_dim is the compact width and obs_out a compact buffer."""
        if self.as_numpy:
            raise ValueError("step_transition: device tensors only (as_numpy=False)")
        out, obs, rewards = self._advance(self._route(actions, own_rows=True), obs_out)
        return (obs.clone() if obs_out is None else obs_out), rewards, out.terminated, out.was_reset

    @property
    def truncated(self):
        """The simulator's u8 truncation flags of the last step (0, 1 time limit, 2 stall), or None
        with the limits off."""
        return self.sim.out.truncated

    def episode_totals(self) -> dict:
        """Totals over the episodes finished since the last reset_episode_totals (episode_stats=True):
        episodes, terminated, truncated, length_sum, return_sum / min / max, return_mean, length_mean
        as Python numbers.  Waits for the stream."""
        if self._episode is None:
            raise ValueError("episode_totals: build the env with episode_stats=True")
        return self._episode.totals()

    def reset_episode_totals(self):
        if self._episode is None:
            raise ValueError("reset_episode_totals: build the env with episode_stats=True")
        self._episode.reset_totals()

    def race_totals(self) -> dict:
        """Totals over the episodes finished since the last reset_race_totals (race_stats=True): the
        fields of f110_race_totals plus progress_mean, lead_mean, length_mean, win_rate and crash_rate
        as Python numbers (race.RaceStats.totals).  Waits for the stream."""
        if self._race is None:
            raise ValueError("race_totals: build the env with race_stats=True")
        return self._race.totals()

    def reset_race_totals(self):
        if self._race is None:
            raise ValueError("reset_race_totals: build the env with race_stats=True")
        self._race.reset_totals()

    def close(self):
        if getattr(self, "_sensor", None) is not None:
            self._sensor.close()
            self._sensor = None
        if getattr(self, "_sobs", None) is not None:
            self._sobs.close()
            self._sobs = None
        if getattr(self, "sim", None) is not None:
            self.sim.close()
            self.sim = None
