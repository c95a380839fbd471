"""Batched DDPG training loop (config 5): rl_training/train_ddpg.py's loop
(:150-216) for N envs per GPU, one process per GPU.

Per vector step, everything on the device:
  ego action    random U(low, high) during warm-up (:162-163), else the actor
                + Gaussian or OU noise (:165); the last `eval_envs` envs are
                evaluation envs (:158-165): the actor's action, noise-free, from step 0
  opponent      gap_follow_action on its previous scan (:168), inside F110VectorEnv; with
                --opponent self a frozen snapshot of the learner's actor instead (its own seat's
                observation, noise-free), refreshed every --selfplay-sync learner updates, in the
                --selfplay-fraction of the envs picked by opponent.selfplay_mask (the others race
                the --opponent-rule); with --opponent pure_pursuit a waypoint follower on the
                reward's centerline at --opponent-speed, aiming --opponent-lookahead ahead
  hold          with --action-repeat K > 1 (a control interval of K simulator steps; no reference
                counterpart) the action is a decision only where the env's block is over: every
                other env's row is overwritten with the action its block began with, on the device,
                whatever wrote it (warm-up draw, actor + noise, eval row).  The actor and the noise
                still run at every simulator step (sigma decays and the OU state advances per step;
                a held row's draw is discarded), as do the opponent, the reward, the episode
                statistics and the eval bookkeeping
  env.step      (:174) with device autoreset (gymnasium NEXT_STEP)
  observation   with --track-obs (no reference counterpart) every observation gains the
                track-relative block of track_obs.TrackObs on the reward's centerline: the ego's speed,
                steering angle, yaw rate and slip, its lateral offset and heading error, the centerline
                --track-preview metres ahead in its own frame and the opponent's gap (one more launch
                inside the step graphs); the learner's obs_dim grows by the block's width, and a
                self-play snapshot sees the same block from its own seat
                with --scan-bins K (no reference counterpart) the observation the policy, the critic,
                the replay and a self-play snapshot see is compact (scan_obs.ScanObs, one more launch
                inside the step graphs): the 1080 ranges pooled into K sectors (--scan-reduce min |
                mean), the last --scan-frames pooled frames stacked --scan-stride steps apart, the pose
                columns kept (or dropped: --scan-drop-poses), the track block after them; the reward,
                the opponents and the statistics keep reading the full rows
                with --sensor-noise / --sensor-noise-rel / --sensor-scale / --sensor-dropout /
                --sensor-blackout / --sensor-quant / --sensor-pose-xy / --sensor-pose-theta LO,HI (no
                reference counterpart) the rows the policy, the critic and the replay see come through a
                randomized sensor (sensor.SensorModel, one more launch inside the step graphs, before the
                scan observation): each parameter is redrawn per env and episode on the device; the
                --eval-envs rows are masked out and stay noise-free, and the reward, the opponents, the
                statistics and a self-play snapshot keep reading the clean rows
  reward        CenterlineSafetyProgressReward (:127-146, :179) on the device
  race          with --race-stats (no reference counterpart) the race outcomes per episode on the
                reward's centerline: progress, lead over the opponent, passes, crash / completed /
                truncated (race.RaceStats, three launches inside the step graphs); the report gains
                progress_mean, lead_mean, win_rate, crash_rate and passes_per_episode, and
                --best-by progress picks best.pt by eval_progress_mean
  remember      (:184) every transition except the reset rows of autoreset steps;
                with --n-step N as N-step returns (device windows in front of the ring);
                with --action-repeat K one row per block: the block's first observation and
                action, its discounted return, the observation after its last step, and the
                effective done 1 - gamma^(k-1) (1 - done) of its k <= K steps (a block ends early
                with its episode; a reset row drops the block and a decision is due right after)
  replay        (:187-188) `updates_per_step` learner updates after warm-up,
                gradients averaged over ranks by RCCL; with --algo td3 the TD3 rule
                (twin critics, target smoothing, delayed actor / target updates)

    python -m torch.distributed.run --nproc-per-node 8 -m f110_gymnasium_ros2_jazzy_amd.train --envs-per-gpu 4096
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from . import distributed as D

# ddpg_config.yaml (agent_hyperparameters, action bounds)
ACTION_LOW = [-0.4189, 0.0]
ACTION_HIGH = [0.4189, 20.0]
# train_ddpg.py:127-146 reward kwargs
REWARD_KW = dict(w_prog=5.0, alive_bonus=0.5, grace_steps_wall=25, grace_steps_opp=175, w_lat=0.25, lat_cap=3.0,
                 near_wall_dist=0.30 / 30, w_wall=0.30, wall_quantile=0.10, opp_safe_dist=0.60, w_opp=0.30,
                 w_rel_lead=0.0)


def add_spawn_args(ap):
    """The start-state randomization flags (F110VectorEnv's spawn_ranges; none given: off)."""
    pair = dict(default=None, metavar="LO,HI")
    ap.add_argument("--spawn-lateral", **pair,
                    help="start this far left of the spawn pose, in metres (a negative LO: --spawn-lateral=-0.3,0.3)")
    ap.add_argument("--spawn-heading", help="start turned by this much, in radians", **pair)
    ap.add_argument("--spawn-speed", help="start rolling at this speed, in m/s", **pair)
    ap.add_argument("--spawn-gap", help="autoresets: the opponent starts this many spawn rows from the ego's", **pair)
    ap.add_argument("--spawn-behind", type=float, default=None, metavar="P",
                    help="--spawn-gap: probability that the opponent starts behind the ego")
    ap.add_argument("--spawn-clearance", type=float, default=None, metavar="M",
                    help="--spawn-lateral: least wall distance accepted at the offset position, in metres")


def spawn_ranges_from_args(args, num_agents: int = 2, opponent_idx: int = 1):
    """F110VectorEnv's spawn_ranges from the --spawn-* flags: one dict per agent (lateral, heading,
    speed and clearance for every car, gap and behind for the opponent only), or None when no flag
    was given.  ValueError for a LO,HI that is no pair of numbers."""
    def pair(name, conv):
        v = getattr(args, name)
        if v is None:
            return None
        try:
            lo, hi = (conv(x) for x in v.split(","))
        except ValueError:
            raise ValueError(f"--{name.replace('_', '-')} takes LO,HI; got {v!r}") from None
        return lo, hi

    every = {k: pair("spawn_" + k, float) for k in ("lateral", "heading", "speed")}
    every["clearance"] = args.spawn_clearance
    opp = {"gap": pair("spawn_gap", int), "behind": args.spawn_behind}
    every, opp = ({k: v for k, v in d.items() if v is not None} for d in (every, opp))
    if not every and not opp:
        return None
    return [{**every, **opp} if a == opponent_idx else dict(every) for a in range(num_agents)]


SENSOR_FLAGS = (("noise", "noise_abs", "additive range noise sigma, in metres"),
                ("noise_rel", "noise_rel", "range-proportional noise sigma, a fraction of the range"),
                ("scale", "scale", "multiplicative range error (1 = exact)"),
                ("dropout", "dropout", "per-beam, per-step probability of no return (the beam reads max range)"),
                ("blackout", "blackout", "width in beams of one blocked sector per episode (it reads 0)"),
                ("quant", "quant", "range quantization step, in metres (0: off)"),
                ("pose_xy", "pose_xy", "sigma of the noise on the x and y columns, in metres"),
                ("pose_theta", "pose_theta", "sigma of the noise on the theta columns, in radians"))


def add_sensor_args(ap):
    """The sensor randomization flags (F110VectorEnv's sensor_ranges; none given: off): each
    parameter is drawn per env and episode, uniform in LO,HI."""
    for flag, _, text in SENSOR_FLAGS:
        ap.add_argument("--sensor-" + flag.replace("_", "-"), default=None, metavar="LO,HI", help="sensor: " + text)


def sensor_ranges_from_args(args):
    """F110VectorEnv's sensor_ranges from the --sensor-* flags, or None when no flag was given.
    ValueError for a LO,HI that is no pair of numbers."""
    ranges = {}
    for flag, name, _ in SENSOR_FLAGS:
        v = getattr(args, "sensor_" + flag)
        if v is None:
            continue
        try:
            lo, hi = (float(x) for x in v.split(","))
        except ValueError:
            raise ValueError(f"--sensor-{flag.replace('_', '-')} takes LO,HI; got {v!r}") from None
        ranges[name] = (lo, hi)
    return ranges or None


class _RowStats:
    """The statistics of the rows [lo, hi) of a step's buffers: an episode.EpisodeStats and a
    race.RaceStats built for hi - lo envs (either may be None)."""

    def __init__(self, lo, hi, episode, race=None):
        self.lo, self.hi, self.episode, self.race = lo, hi, episode, race

    def update(self, rew, obs, term, trunc, was_reset):
        rows = slice(self.lo, self.hi)
        term, trunc, was_reset = term[rows], None if trunc is None else trunc[rows], was_reset[rows]
        self.episode.update(rew[rows], term, trunc, was_reset)
        if self.race is not None:
            self.race.update(obs[rows], term, trunc, was_reset)

    def totals_and_reset(self):
        """[episode totals or None, race totals or None] since the last call (waits for the stream)."""
        out = [None if s is None else s.totals() for s in (self.episode, self.race)]
        for s in (self.episode, self.race):
            if s is not None:
                s.reset_totals()
        return out


class VectorTrainer:
    """One rank's share of the batched train_ddpg loop."""

    def __init__(self, envs_per_rank: int, map_name: str = "Spielberg_map", batch_size: int = 4096,
                 memory_size: int = 1 << 20, warmup_steps: int = 1000, updates_per_step: int = 1, seed: int = 42,
                 device=None, env_offset: int = 0, rank_seed: int = 0, graphs: bool = True,
                 max_episode_steps: int | None = None, stall_speed: float = 0.0, stall_steps: int | None = None,
                 noise_type: str = "gaussian", eval_envs: int = 0, ou_reset: bool = False, n_step: int = 1,
                 algo: str = "ddpg", policy_delay: int = 2, policy_noise: float = 0.2, noise_clip: float = 0.5,
                 opponent: str = "gap_follow", selfplay_sync: int = 1000, selfplay_fraction: float = 1.0,
                 opponent_speed=None, opponent_lookahead: float | None = None, opponent_rule: str = "gap_follow",
                 action_repeat: int = 1, race_stats: bool = False, track_obs: bool = False, track_preview=None,
                 scan_bins: int | None = None, scan_frames: int = 1, scan_stride: int = 1, scan_reduce: str = "min",
                 scan_keep_poses: bool = True, spawn_ranges=None, spawn_seed: int | None = None, sensor_ranges=None,
                 sensor_seed: int | None = None):
        # action_repeat and the opponent arguments: ValueError before anything is built
        from .opponent import check_pursuit_speed
        from .replay import check_action_repeat
        if check_action_repeat(action_repeat) > 1 and int(n_step) > 1:
            raise ValueError("action_repeat > 1 with n_step > 1 is not supported; use one of the two")
        if opponent not in ("gap_follow", "self", "pure_pursuit"):
            raise ValueError(f"opponent must be 'gap_follow', 'self' or 'pure_pursuit'; got {opponent!r}")
        if opponent_rule not in ("gap_follow", "pure_pursuit"):
            raise ValueError(f"opponent_rule must be 'gap_follow' or 'pure_pursuit'; got {opponent_rule!r}")
        if opponent_lookahead is not None and not float(opponent_lookahead) > 0.0:
            raise ValueError(f"opponent_lookahead must be > 0; got {opponent_lookahead!r}")
        check_pursuit_speed(opponent_speed, envs_per_rank)
        if int(selfplay_sync) != selfplay_sync or selfplay_sync < 1:
            raise ValueError(f"selfplay_sync must be an integer >= 1; got {selfplay_sync!r}")
        if not 0.0 <= float(selfplay_fraction) <= 1.0:
            raise ValueError(f"selfplay_fraction must be in [0, 1]; got {selfplay_fraction!r}")
        if track_preview is not None and not track_obs:
            raise ValueError("track_preview needs track_obs")
        tobs_kw = None  # F110VectorEnv's track_obs argument
        if track_obs:
            from .track_obs import MAX_PREVIEW
            tobs_kw = {} if track_preview is None else {"preview": tuple(float(d) for d in track_preview)}
            if len(tobs_kw.get("preview", ())) > MAX_PREVIEW or any(not d > 0.0 for d in tobs_kw.get("preview", ())):
                raise ValueError(f"track_preview takes at most {MAX_PREVIEW} distances > 0; got {track_preview!r}")
        sobs_kw = None  # F110VectorEnv's scan_obs argument
        if scan_bins is None:
            if (scan_frames, scan_stride, scan_reduce, bool(scan_keep_poses)) != (1, 1, "min", True):
                raise ValueError("scan_frames, scan_stride, scan_reduce and scan_keep_poses need scan_bins")
        else:
            from . import _lib
            from .scan_obs import scan_obs_params
            sobs_kw = dict(n_bins=scan_bins, n_frames=scan_frames, stride=scan_stride, reduce=scan_reduce,
                           keep_mid=bool(scan_keep_poses))
            scan_obs_params(_lib.default_config().n_beams, **sobs_kw)  # a value out of range: ValueError
        if sensor_ranges is not None:  # an unknown name, a value out of range: ValueError
            from . import _lib, sensor
            if not isinstance(sensor_ranges, dict):
                raise ValueError("sensor_ranges must be None or a dict {name: (lo, hi)}")
            sensor.sensor_ranges(_lib.default_config().n_beams, **sensor_ranges)
        elif sensor_seed is not None:
            raise ValueError("sensor_seed needs sensor_ranges")
        self.selfplay = opponent == "self"
        self.selfplay_sync, self.selfplay_fraction = int(selfplay_sync), float(selfplay_fraction)
        if self.selfplay:
            from . import ddpg
            if torch.device(device or "cuda").type != "cuda" or not (ddpg.FUSED and ddpg.EXPLICIT):
                raise ValueError("opponent='self' needs the explicit learner path (a HIP device, F110_DDPG_FUSED "
                                 "and F110_DDPG_EXPLICIT on): the policy opponent has no torch path")
        from .ddpg import DDPGLearner
        from .maps import MAP_DIR
        from .reward import BatchedCenterlineReward, CenterlineTrack
        from .vector_env import F110VectorEnv
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self.N = int(envs_per_rank)
        self.eval_envs = int(eval_envs)
        if not 0 <= self.eval_envs < self.N:
            raise ValueError(f"eval_envs must be in [0, {self.N}); got {eval_envs}")
        self.ou_reset = bool(ou_reset)
        cl = np.load(os.path.join(MAP_DIR, map_name.replace("_map", "") + "_centerline.npz"))
        self.track = CenterlineTrack(cl["xy"], cl["w_right"], cl["w_left"], device=self.device.index or 0)
        self.reward_fn = BatchedCenterlineReward(self.N, dt=0.01, progress=self.track, device=self.device,
                                                 **REWARD_KW)
        # episode limits (device truncation): with any of them on the env also keeps the episode
        # statistics on the device (one kernel pair per step, inside the step graphs)
        # With evaluation envs the trainer keeps the statistics itself, one EpisodeStats over the
        # training rows and one over the eval rows (contiguous row ranges of the step's buffers)
        # race_stats: the race outcomes beside them (race.RaceStats on the reward's centerline, three
        # more launches per step, kept the same way: the env's own, or one per row range)
        self.race_stats = bool(race_stats)
        self.episode_stats = bool(max_episode_steps or stall_steps or self.eval_envs)
        env_kw = dict(map=map_name, num_agents=2, seed=seed, device=self.device, env_offset=env_offset,
                      reward_fn=self.reward_fn, infos="minimal", max_episode_steps=max_episode_steps,
                      stall_speed=stall_speed, stall_steps=stall_steps,
                      episode_stats=self.episode_stats and not self.eval_envs)
        if self.race_stats and not self.eval_envs:
            env_kw["race_stats"] = True
        if tobs_kw is not None:  # on the reward's centerline (reward_fn.progress)
            env_kw["track_obs"] = tobs_kw
        if sobs_kw is not None:  # the learner, the replay and the snapshot see the compact rows
            env_kw["scan_obs"] = sobs_kw
        if spawn_ranges is not None:  # start states drawn on the device, evaluation envs included (keyed by env id)
            env_kw.update(spawn_ranges=spawn_ranges, spawn_seed=spawn_seed)
        if sensor_ranges is not None:  # the learner and the replay see the rows through the sensor; the evaluation
            # envs (the last eval_envs rows) are masked out and stay noise-free; a snapshot sees clean rows
            mask = np.ones(self.N, np.uint8)
            mask[self.N - self.eval_envs:] = 0
            env_kw.update(sensor_ranges=sensor_ranges, sensor_seed=sensor_seed, sensor_mask=mask)
        learner = lambda obs_dim: DDPGLearner(  # noqa: E731
            obs_dim=obs_dim, act_dim=2, action_low=ACTION_LOW, action_high=ACTION_HIGH, gamma=0.99, tau=0.005,
            actor_lr=1e-4, critic_lr=1e-3, memory_size=memory_size, batch_size=batch_size, alpha=0.6, beta=0.4,
            priority_epsilon=1e-5, noise_sigma_start=0.20, noise_sigma_min=0.02, noise_decay=0.9995, seed=seed,
            device=self.device, max_add=self.N, graphs=graphs, noise_type=noise_type, n_step=n_step, algo=algo,
            policy_delay=policy_delay, policy_noise=policy_noise, noise_clip=noise_clip,
            action_repeat=int(action_repeat))
        # the waypoint follower drives on the reward's centerline (self.track)
        pursuit = opponent == "pure_pursuit" or (self.selfplay and selfplay_fraction < 1.0
                                                 and opponent_rule == "pure_pursuit")
        pursuit_kw = dict(opponent_track=self.track, opponent_speed=opponent_speed,
                          opponent_params={} if opponent_lookahead is None else
                          {"lookahead": float(opponent_lookahead)}) if pursuit else {}
        self.opp = None
        if self.selfplay:
            # the snapshot needs the learner's actor, the env the snapshot: the learner comes first (its
            # obs_dim from the library's beam count), and the snapshot starts as the initial actor, which
            # the warm-up is raced against
            from . import _lib
            from .opponent import PolicyOpponent, selfplay_mask
            tail = 0
            if tobs_kw is not None:  # the width the env will add (two agents: with the gap columns)
                from .track_obs import track_obs_params, track_obs_width
                tail = track_obs_width(track_obs_params(**tobs_kw).n_preview, True)
            beams = _lib.default_config().n_beams
            width = beams + 4 * 2 + tail
            if sobs_kw is not None:
                from .scan_obs import ScanObs, scan_obs_width
                width = scan_obs_width(beams, 4 * 2, tail, **sobs_kw)
            self.agent = learner(width)
            if self.agent.explicit is None:
                raise ValueError("opponent='self' needs a learner with the explicit path")
            self.opp = PolicyOpponent(self.agent.actor, self.N, self.device)
            if sobs_kw is not None:  # the snapshot's own ring, over its own seat's full rows
                self.opp.set_scan_obs(ScanObs(self.N, beams, 4 * 2, tail, device=self.device, **sobs_kw))
            mixed = self.selfplay_fraction < 1.0
            self.env = F110VectorEnv(self.N, opponent="mixed" if mixed else "policy", opponent_policy=self.opp,
                                     opponent_mask=selfplay_mask(self.N, env_offset, self.selfplay_fraction)
                                     if mixed else None, opponent_rule=opponent_rule, **pursuit_kw, **env_kw)
            if self.env.single_observation_space.shape[0] != self.agent.obs_dim:
                raise ValueError("the env's observation size differs from the learner's")
            if tobs_kw is not None:  # the snapshot's own seat, now that the simulator exists
                from .track_obs import TrackObs
                self.opp.set_track_obs(TrackObs(self.env.sim, self.track, seat=self.env.opponent_idx, other=0,
                                                **tobs_kw))
        else:
            self.env = F110VectorEnv(self.N, opponent=opponent, **pursuit_kw, **env_kw)
        self._synced_at = 0  # the learner update index of the snapshot's last load
        # the statistics the report reads, as (report prefix, group): the env's own, or with evaluation
        # envs one group over the training rows and one over the eval rows, which _transition updates
        self._eval_mask = self.train_stats = self.eval_stats = self.train_race = self.eval_race = None
        self._stats = [("", _RowStats(0, self.N, self.env._episode, self.env._race))]
        if self.eval_envs:
            from .episode import EpisodeStats
            from .race import RaceStats
            k = self.N - self.eval_envs
            self._eval_mask = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
            self._eval_mask[k:] = 1
            self._stats = [(prefix, _RowStats(
                lo, hi, EpisodeStats(hi - lo, device=self.device),
                RaceStats(hi - lo, self.track, self.env.sim.B, ego_idx=0, opponent_idx=self.env.opponent_idx,
                          device=self.device) if self.race_stats else None))
                for prefix, lo, hi in (("", 0, k), ("eval_", k, self.N))]
            (_, tg), (_, eg) = self._stats
            self.train_stats, self.train_race, self.eval_stats, self.eval_race = tg.episode, tg.race, eg.episode, eg.race
        if not self.selfplay:
            self.agent = learner(self.env.single_observation_space.shape[0])
        self.warmup = int(warmup_steps)
        self.updates_per_step = int(updates_per_step)
        # HIP graphs per vector step once the learner's eager warm-up updates are done (explicit
        # learner, one update per step): even / odd steps have their own captures, which swap the two
        # fixed observation buffers and the learner's two noise-state slots; one graph per step on
        # one rank, three (split at the gradient all-reduces) on several.  The captures are keyed by
        # (parity, actor step): every DDPG update is an actor step; a delayed-actor update that is
        # none has two graphs on several ranks
        self.step_graphs = bool(graphs) and os.environ.get("F110_STEP_GRAPH", "1") != "0"
        self._sg = {}
        self._sg_parity = 0
        self._sg_obs = None
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed * 1000003 + rank_seed)
        self._low = torch.tensor(ACTION_LOW, device=self.device)
        self._high = torch.tensor(ACTION_HIGH, device=self.device)
        self.obs, self.info = self.env.reset(seed=seed + rank_seed)
        if self.train_race is not None:  # the reset observation (its full rows) starts every env's race
            for _, g in self._stats:
                g.race.begin(self.env.full_obs[g.lo:g.hi])
        self.global_step = 0
        self.last = None

    def step(self):
        """One vector step of the loop (train_ddpg.py:160-192).  Returns the
        step's rewards (float64) and terminated flags (uint8): device buffers
        valid until the next step()."""
        if self.global_step < self.warmup:  # :162-163
            u = torch.rand(self.N, 2, generator=self._gen, device=self.device)
            act = self._low + u * (self._high - self._low)
            if self.eval_envs:  # an eval episode bypasses the warm-up's random actions (:160-165)
                k = self.N - self.eval_envs
                act[k:] = self.agent.choose_action(self.obs, training=False)[k:]
        elif self._graph_ready():
            return self._step_graphed()
        else:  # the actions land in the env's action rows (no copy in the step)
            act = self._explore(self.obs)
        next_obs, rew, term, was_reset = self._transition(self.obs, act, None)
        if self.global_step >= self.warmup:
            for _ in range(self.updates_per_step):
                self.last = self.agent.replay()
        self._selfplay_sync()
        self.obs = next_obs
        self.global_step += 1
        return rew, term

    def _selfplay_sync(self):
        """After every selfplay_sync-th completed learner update the snapshot takes the actor's
        weights: one flat copy on the current stream, on the host side of the step and outside any
        captured graph.  The snapshot's buffers are fixed, so the next step's opponent forward --
        eager or a replayed step graph -- is the first to use them."""
        if self.opp is None:
            return
        n = self.agent.global_step
        if n != self._synced_at and n % self.selfplay_sync == 0:
            self.opp.load(self.agent.actor)
            self._synced_at = n

    def save_checkpoint(self, filename: str = "best.pt"):
        """DDPGLearner.save_model (same keys); with self-play also "opponent_actor", the snapshot's
        state dict, so a resumed run races the same opponent."""
        self.agent.save_model(filename, extra={"opponent_actor": self.opp.state_dict()} if self.opp else None)

    def load_checkpoint(self, filename: str = "best.pt") -> bool:
        """DDPGLearner.load_model, then the snapshot from "opponent_actor" (a file without the key
        leaves the snapshot as it is)."""
        if not self.agent.load_model(filename):
            return False
        if self.opp is not None:
            ckpt = torch.load(os.path.join(self.agent.path, filename), map_location=self.device, weights_only=True)
            if "opponent_actor" in ckpt:
                self.opp.load_state_dict(ckpt["opponent_actor"])
        return True

    def _graph_ready(self) -> bool:
        ag = self.agent
        return (self.step_graphs and ag.explicit is not None and ag.graphs and self.updates_per_step == 1 and
                ag._ready and ag._eager_left == 0 and ag._graphs is None and self.env.agent_actions() is not None)

    def _explore(self, obs):
        """The step's actions into the env's action rows: the eval rows noise-free, the others with
        the learner's noise; with ou_reset the rows the previous step reset start from x = 0 (the
        simulator's was_reset buffer, which this step's env.step rewrites only afterwards)."""
        reset = self.env.sim.out.was_reset if self.ou_reset else None
        return self.agent.choose_action(obs, training=True, out=self.env.agent_actions(), eval_mask=self._eval_mask,
                                        reset=reset)

    def _transition(self, obs_in, act, obs_out):
        """hold (action_repeat > 1: held actions over the rows whose decision is not due, in place
        -- in the env's own action rows when act is that view, so the step still copies nothing),
        env.step, the episode statistics of the two row ranges (eval_envs > 0) and remember."""
        act = self.agent.hold_env(obs_in, act)
        nxt, rew, term, was_reset = self.env.step_transition(act, obs_out=obs_out)
        if self.eval_envs:  # (the race statistics on the obs buffer the reward saw: the full rows)
            for _, g in self._stats:
                g.update(rew, self.env.full_obs, term, self.env.truncated, was_reset)
        # NEXT_STEP autoreset: a reset row's obs is the previous episode's last
        # observation and its next_obs the new episode's first -- not a transition
        # (remember_env skips the rows with was_reset != 0); eval transitions are stored like any
        # other (train_ddpg.py:184 remembers unconditionally).  n_step > 1: the step goes into the
        # learner's n-step windows, which also end at this step's truncated rows; action_repeat > 1:
        # into its action-repeat blocks (obs_in and act were latched by the hold where a block began)
        self.agent.remember_env(obs_in, act, rew, nxt, term, was_reset, truncated=self.env.truncated)
        return nxt, rew, term, was_reset

    def _head(self, obs_in, obs_out, phase_a):
        """A vector step after the warm-up up to the first all-reduce, as captured:
        choose_action (noise in the head launch), env step + reward, replay add,
        the learner update's first phase (sample, critic loss and gradients)."""
        ag = self.agent
        act = self._explore(obs_in)
        _, rew, term, _ = self._transition(obs_in, act, obs_out)
        phase_a()
        return rew, term

    def _capture(self, p, actor_step=True):
        """The step graphs of one (parity, update kind): its own learner phases and loss outputs
        (ddpg._phases per parity: the two captures share a memory pool,
        so one parity's outputs must not be the other's scratch).  One rank: the
        whole step is one graph.  Several ranks: three graphs split at the two
        gradient-bucket all-reduces, which run eagerly (RCCL) between the replays (two graphs and
        one all-reduce for an update that is no actor step)."""
        ag = self.agent
        bufs = self._sg_obs
        phases, out = ag._phases(actor_step)
        ret = {}

        def head():
            ret["v"] = self._head(bufs[p], bufs[1 - p], phases[0])

        def whole():
            head()
            for ph in phases[1:]:
                ph()
        segs = [head, *phases[1:]] if ag.distributed else [whole]
        cur = torch.cuda.current_stream(self.device)
        graphs = []
        for seg in segs:  # capture records, it does not run
            g = torch.cuda.CUDAGraph()
            ag._side.wait_stream(cur)
            with torch.cuda.graph(g, pool=self._sg_pool, stream=ag._side):
                seg()
            cur.wait_stream(ag._side)
            graphs.append(g)
        return graphs, out, ret["v"]

    def _step_graphed(self):
        """step() as replays of the parity's captured graphs (captured on its
        first use: the capture runs the Python side once, which is this step's
        host bookkeeping; before later replays the learner repeats it)."""
        ag = self.agent
        p = self._sg_parity
        if self._sg_obs is None:
            self._sg_obs = [torch.empty_like(self.obs), torch.empty_like(self.obs)]
            self._sg_pool = torch.cuda.graph_pool_handle()
        bufs = self._sg_obs
        if self.obs.data_ptr() != bufs[p].data_ptr():
            bufs[p].copy_(self.obs)
        actor_step = ag.is_actor_step()  # the host picks the capture by the learner's update index
        if (p, actor_step) not in self._sg:
            self._sg[p, actor_step] = self._capture(p, actor_step)
        else:
            ag.step_graph_replay(self.N)
        graphs, out, ret = self._sg[p, actor_step]
        ag._run_phases([g.replay for g in graphs])  # several ranks: with the bucket all-reduces between
        self.last = ag._update_result(out, actor_step)
        self._selfplay_sync()
        self.obs = bufs[1 - p]
        self._sg_parity ^= 1
        self.global_step += 1
        return ret

    def close(self):
        self.env.close()
        self.track.close()


# the report of one group's totals: (the count's report key, the totals that ride in the all-reduce, the count
# first, and the report key of each other total's mean per episode); "{p}" is the group's prefix
EPISODE_REPORT = ("{p}episodes", ("episodes", "return_sum", "length_sum"), ("{e}return_mean", "{e}length_mean"))
RACE_REPORT = ("{p}race_episodes", ("episodes", "progress_sum", "lead_sum", "ahead_at_end", "ego_crashes", "passes"),
               ("{p}progress_mean", "{p}lead_mean", "{p}win_rate", "{p}crash_rate", "{p}passes_per_episode"))
RACE_REPORT_SUMS = RACE_REPORT[1]


def episode_report(tr: VectorTrainer, world: int = 1) -> dict:
    """The episodes finished since the last report, summed over ranks on the host (print time only),
    then cleared: episodes, episode_return_mean, episode_length_mean.  With evaluation envs these
    three cover the training rows, and eval_episodes, eval_return_mean, eval_length_mean the eval rows.
    With race_stats also race_episodes, progress_mean, lead_mean, win_rate, crash_rate and
    passes_per_episode (and their eval_ twins), from the race totals in the same all-reduce; a
    trainer that keeps race statistics only (no limits, no evaluation envs) reports those alone."""
    totals = [(prefix, *g.totals_and_reset()) for prefix, g in tr._stats]
    # one vector, the same layout on every rank: every group's episode sums, then every group's race sums
    parts = [(prefix, EPISODE_REPORT, ep) for prefix, ep, _ in totals if ep is not None] + \
            [(prefix, RACE_REPORT, race) for prefix, _, race in totals if race is not None]
    v = [float(tot[k]) for _, (_, sums, _), tot in parts for k in sums]
    if world > 1:
        import torch.distributed as dist
        w = torch.tensor(v, dtype=torch.float64)
        if dist.get_backend() != "gloo":
            w = w.to(tr.device)
        dist.all_reduce(w)
        v = w.tolist()
    rep = {}
    for prefix, (count, sums, means), _ in parts:
        n, names = int(v[0]), dict(p=prefix, e=prefix or "episode_")
        rep[count.format(**names)] = n
        rep.update({key.format(**names): x / n if n else None for key, x in zip(means, v[1:len(sums)])})
        v = v[len(sums):]
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs-per-gpu", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--memory", type=int, default=1 << 20)
    ap.add_argument("--updates-per-step", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--max-episode-steps", type=int, default=0, help="time limit per episode in steps (0: none)")
    ap.add_argument("--stall-speed", type=float, default=0.0, help="ego speed below which a step counts as standing")
    ap.add_argument("--stall-steps", type=int, default=0, help="standing steps in a row that truncate (0: none)")
    ap.add_argument("--noise", choices=("gaussian", "ou"), default="gaussian", help="exploration noise")
    ap.add_argument("--eval-envs", type=int, default=0, help="noise-free evaluation envs per GPU (the last K)")
    ap.add_argument("--ou-reset", action="store_true", help="zero an env's OU state when its episode resets")
    ap.add_argument("--n-step", type=int, default=1, help="n-step returns in the replay (1: one-step targets)")
    ap.add_argument("--action-repeat", type=int, default=1,
                    help="hold each action for K simulator steps and store one replay row per block (1: off)")
    ap.add_argument("--algo", choices=("ddpg", "td3"), default="ddpg", help="the learner's update rule")
    ap.add_argument("--policy-delay", type=int, default=2, help="td3: actor / target update every N-th update")
    ap.add_argument("--policy-noise", type=float, default=0.2,
                    help="td3: target smoothing noise, in units of the action half-range")
    ap.add_argument("--noise-clip", type=float, default=0.5, help="td3: clip of the smoothing noise, same units")
    ap.add_argument("--opponent", choices=("gap_follow", "self", "pure_pursuit"), default="gap_follow",
                    help="the car the learner races: the rule-based gap follower, a frozen copy of its own actor, "
                         "or a pure-pursuit waypoint follower on the centerline")
    ap.add_argument("--opponent-speed", type=float, default=None,
                    help="pure_pursuit: the follower's speed in m/s (default: the library's 4.0)")
    ap.add_argument("--opponent-lookahead", type=float, default=None,
                    help="pure_pursuit: metres of centerline it aims ahead (default: the library's 1.2)")
    ap.add_argument("--opponent-rule", choices=("gap_follow", "pure_pursuit"), default="gap_follow",
                    help="self with --selfplay-fraction < 1: the rule opponent of the other envs")
    ap.add_argument("--selfplay-sync", type=int, default=1000,
                    help="self: refresh the frozen copy every K learner updates")
    ap.add_argument("--selfplay-fraction", type=float, default=1.0,
                    help="self: share of the envs that race the copy (the others race gap_follow)")
    ap.add_argument("--save-dir", default=None, help="rank 0 saves best.pt here when the --best-by figure improves")
    ap.add_argument("--race-stats", action="store_true",
                    help="race outcomes on the device: progress, lead, passes, win and crash rates in the report")
    ap.add_argument("--best-by", choices=("return", "progress"), default="return",
                    help="what picks best.pt: eval_return_mean, or eval_progress_mean (needs --race-stats and "
                         "--eval-envs)")
    ap.add_argument("--track-obs", action="store_true",
                    help="append the track-relative block to every observation: own speed, steering, yaw rate and "
                         "slip, lateral offset and heading error, a centerline preview and the opponent's gap")
    ap.add_argument("--track-preview", default=None, metavar="1,2,4,8",
                    help="--track-obs: the preview distances in metres along the centerline (at most 8)")
    ap.add_argument("--scan-bins", type=int, default=None, metavar="K",
                    help="compact observation: pool the 1080 ranges into K sectors on the device (off by default)")
    ap.add_argument("--scan-frames", type=int, default=None, metavar="F",
                    help="--scan-bins: stack the last F pooled frames, newest first (1..8, default 1)")
    ap.add_argument("--scan-stride", type=int, default=None, metavar="S",
                    help="--scan-bins: simulator steps between stacked frames (1..16, default 1)")
    ap.add_argument("--scan-reduce", choices=("min", "mean"), default=None,
                    help="--scan-bins: a sector's value, the minimum (default) or the mean of its ranges")
    ap.add_argument("--scan-drop-poses", action="store_true",
                    help="--scan-bins: drop the map-frame pose columns from the compact observation")
    add_spawn_args(ap)
    add_sensor_args(ap)
    args = ap.parse_args()
    try:
        spawn_ranges = spawn_ranges_from_args(args)
        sensor_ranges = sensor_ranges_from_args(args)
    except ValueError as exc:
        ap.error(str(exc))
    if args.track_preview is not None and not args.track_obs:
        ap.error("--track-preview needs --track-obs")
    if args.scan_bins is None and (args.scan_frames is not None or args.scan_stride is not None
                                   or args.scan_reduce is not None or args.scan_drop_poses):
        ap.error("--scan-frames, --scan-stride, --scan-reduce and --scan-drop-poses need --scan-bins")
    if args.best_by == "progress" and not (args.race_stats and args.eval_envs > 0):
        ap.error("--best-by progress needs --race-stats and --eval-envs")
    rank, world, local = D.init()
    torch.cuda.set_device(D.local_device_index(local))
    shard = D.shard_range(args.envs_per_gpu * world, world, rank)
    tr = VectorTrainer(shard.count, batch_size=args.batch, memory_size=args.memory, warmup_steps=args.warmup,
                       updates_per_step=args.updates_per_step, seed=args.seed, env_offset=shard.offset,
                       rank_seed=rank, max_episode_steps=args.max_episode_steps, stall_speed=args.stall_speed,
                       stall_steps=args.stall_steps, noise_type=args.noise, eval_envs=args.eval_envs,
                       ou_reset=args.ou_reset, n_step=args.n_step, algo=args.algo, policy_delay=args.policy_delay,
                       policy_noise=args.policy_noise, noise_clip=args.noise_clip, opponent=args.opponent,
                       selfplay_sync=args.selfplay_sync, selfplay_fraction=args.selfplay_fraction,
                       opponent_speed=args.opponent_speed, opponent_lookahead=args.opponent_lookahead,
                       opponent_rule=args.opponent_rule, action_repeat=args.action_repeat,
                       race_stats=args.race_stats, track_obs=args.track_obs,
                       track_preview=None if args.track_preview is None else
                       [float(d) for d in args.track_preview.split(",") if d.strip()],
                       scan_bins=args.scan_bins, scan_frames=args.scan_frames or 1, scan_stride=args.scan_stride or 1,
                       scan_reduce=args.scan_reduce or "min", scan_keep_poses=not args.scan_drop_poses,
                       spawn_ranges=spawn_ranges, sensor_ranges=sensor_ranges)
    best = -float("inf")
    t0 = time.perf_counter()
    ret = torch.zeros(shard.count, device=tr.device, dtype=torch.float64)
    for k in range(args.steps):
        rew, term = tr.step()
        ret += rew
        if (k + 1) % 500 == 0:
            # (every rank: a host all-reduce)
            ep = episode_report(tr, world) if tr.episode_stats or tr.race_stats else {}
            ev = ep.get("eval_progress_mean" if args.best_by == "progress" else "eval_return_mean")
            if rank == 0 and args.save_dir and ev is not None and ev > best:  # train_ddpg.py:213-216, batched
                best = ev
                tr.agent.path = args.save_dir
                tr.save_checkpoint("best.pt")
            if rank == 0:
                st = tr.last or {}
                print(json.dumps({"step": k + 1, "algo": args.algo, "obs_dim": tr.agent.obs_dim,
                                  "env_steps_per_s": shard.count * world * (k + 1) / (time.perf_counter() - t0),
                                  "critic_loss": float(st["critic_loss"]) if st else None,
                                  "mean_return": float(ret.mean()), **ep}), flush=True)
    tr.close()
    D.shutdown()


if __name__ == "__main__":
    main()
