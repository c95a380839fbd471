"""Opponents on the device.

Rule-based: gap_follow_action (rl_training/utils/gap_follow.py:3-58) for a
batch of float32 scans through libf110's f110_gap_follow, bit-exact with the
reference's NumPy float32 arithmetic.  train_ddpg.py:168 computes it on the
host from the previous step's info["scans"][1];
F110VectorEnv(opponent="gap_follow") keeps that loop on the GPU.

``pure_pursuit`` is the other rule: a waypoint follower on a CenterlineTrack (f110_pure_pursuit; no
reference counterpart), each car aiming one lookahead ahead of its projection onto the centerline;
``host_pure_pursuit`` is its host statement over NumPy arrays.
F110VectorEnv(opponent="pure_pursuit") runs it on the opponent's pose group of every step's obs.

Self-play (no reference counterpart): ``agent_obs`` packs the flat observation
from any agent's seat (f110_agent_obs), ``PolicyOpponent`` holds a frozen copy
of an Actor and writes its actions into the opponent's rows of the env's action
buffer (the learner GEMMs, then f110_policy_head_rows), and ``selfplay_mask``
is the fixed per-env rule that splits the envs between the two opponents.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._dev import as_device, device_track, ptr, row_stride
from ._dev import stream as current_stream

ANGLE_MIN = -math.pi / 2          # gap_follow.py:44 defaults
ANGLE_INCREMENT = math.pi / 1080


def gap_follow(scans: torch.Tensor, out: torch.Tensor | None = None, angle_min: float = ANGLE_MIN,
               angle_increment: float = ANGLE_INCREMENT, return_gaps: bool = False, stream=None):
    """scans: float32 device tensor [M, B] (rows may be strided, e.g.
    ``sim.out.scans[:, 1]``).  Returns actions [M, 2] float32 (steer, speed),
    written into ``out`` if given (rows may be strided), plus the chosen gaps
    [M, 2] int32 when ``return_gaps``."""
    if scans.dim() != 2 or scans.dtype != torch.float32 or scans.device.type != "cuda" or scans.stride(1) != 1:
        raise ValueError("scans must be a float32 cuda tensor [M, B] with unit stride along beams")
    M, B = scans.shape
    if out is None:
        out = torch.empty(M, 2, dtype=torch.float32, device=scans.device)
    if out.shape != (M, 2) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != scans.device:
        raise ValueError("out must be a float32 [M, 2] tensor on the scans' device with unit column stride")
    gaps = torch.empty(M, 2, dtype=torch.int32, device=scans.device) if return_gaps else None
    _lib.check(_lib.load().f110_gap_follow(ptr(scans), M, row_stride(scans), B, float(angle_min),
                                           float(angle_increment), ptr(out), row_stride(out), ptr(gaps),
                                           current_stream(scans.device, stream)), "f110_gap_follow")
    return (out, gaps) if return_gaps else out


# ------------------------------------------------------------- pure pursuit --
PURSUIT_FIELDS = ("lookahead", "wheelbase", "speed", "a_lat", "v_floor", "steer_limit", "direction")


def check_pursuit_speed(speed, n_envs):
    """opponent_speed (an env's or a trainer's argument): None, one number or one per env, finite
    and >= 0; host values only."""
    if speed is None:
        return
    sp = np.asarray(speed, dtype=np.float64)
    if sp.shape not in ((), (int(n_envs),)):
        raise ValueError(f"opponent_speed must be one number or an array [{int(n_envs)}]")
    if not (np.isfinite(sp).all() and (sp >= 0.0).all()):
        raise ValueError("opponent_speed must be finite and >= 0")


def pursuit_params(**params) -> "_lib.F110PursuitParams":
    """f110_default_pursuit_params with ``params`` (lookahead, wheelbase, speed, a_lat, v_floor,
    steer_limit, direction) on top; an unknown name is a ValueError.  The values themselves are
    checked by the library at the call."""
    p = _lib.F110PursuitParams()
    _lib.load().f110_default_pursuit_params(ctypes.byref(p))
    for k, v in params.items():
        if k not in PURSUIT_FIELDS:
            raise ValueError(f"unknown pure-pursuit parameter {k!r} (known: {', '.join(PURSUIT_FIELDS)})")
        if k == "direction":
            if v not in (1, -1):
                raise ValueError(f"direction must be +1 or -1; got {v!r}")
            p.direction = int(v)
        else:
            setattr(p, k, float(v))
    return p


def pure_pursuit(poses: torch.Tensor, track, out: torch.Tensor | None = None, row_speed: torch.Tensor | None = None,
                 row_mask: torch.Tensor | None = None, return_aux: bool = False, stream=None, **params):
    """Pure-pursuit actions for M cars (f110_pure_pursuit).  poses: float32 device tensor [M, >= 3]
    whose rows start with (x, y, yaw) (rows may be strided, e.g. ``obs[:, B + 4:B + 8]``, agent 1's
    pose group of a step's obs); track: a device reward.CenterlineTrack.  Returns actions [M, 2]
    float32 (steer, speed), written into ``out`` if given (rows may be strided, e.g. ``act[:, 1]`` of
    an [M, A, 2] action buffer), plus aux [M, 4] float64 (s_proj, t, target x, y) when
    ``return_aux``.  row_speed: float64 [M] per-row speeds (None: ``speed`` for all); row_mask:
    uint8 [M], rows with 0 keep their values (None: every row); params: see pursuit_params."""
    if (poses.dim() != 2 or poses.dtype != torch.float32 or poses.device.type != "cuda" or poses.shape[1] < 3
            or poses.stride(1) != 1):
        raise ValueError("poses must be a float32 cuda tensor [M, >= 3] with unit stride along the pose")
    M = poses.shape[0]
    device_track(track, poses.device, "track", user="the poses")
    if out is None:
        out = torch.empty(M, 2, dtype=torch.float32, device=poses.device)
    if out.shape != (M, 2) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != poses.device:
        raise ValueError("out must be a float32 [M, 2] tensor on the poses' device with unit column stride")
    for name, t, dt in (("row_speed", row_speed, torch.float64), ("row_mask", row_mask, torch.uint8)):
        if t is not None and (t.dtype != dt or t.shape != (M,) or not t.is_contiguous() or t.device != poses.device):
            raise ValueError(f"{name} must be a contiguous {dt} [M] tensor on the poses' device")
    aux = torch.empty(M, 4, dtype=torch.float64, device=poses.device) if return_aux else None
    p = pursuit_params(**params)
    _lib.check(_lib.load().f110_pure_pursuit(track.handle, ctypes.byref(p), ptr(poses), M, row_stride(poses),
                                             ptr(row_speed), ptr(row_mask), ptr(out), row_stride(out), ptr(aux),
                                             current_stream(poses.device, stream)), "f110_pure_pursuit")
    return (out, aux) if return_aux else out


def host_pure_pursuit(poses: np.ndarray, track, out: np.ndarray | None = None, row_speed=None, row_mask=None,
                      return_aux: bool = False, **params):
    """f110_host_pure_pursuit over NumPy arrays: the host statement of pure_pursuit, for tests
    without a GPU (track: any CenterlineTrack, ``device=None`` included).  poses: float32 [M, >= 3]
    and out: float32 [M, 2] may be strided along rows (unit stride inside a row)."""
    poses = np.asarray(poses)
    if poses.ndim != 2 or poses.dtype != np.float32 or poses.shape[1] < 3 or (poses.size and poses.strides[1] != 4):
        raise ValueError("poses must be a float32 array [M, >= 3] with unit stride along the pose")
    M = poses.shape[0]
    if not getattr(track, "handle", None):
        raise ValueError("track must be an open reward.CenterlineTrack")
    if out is None:
        out = np.empty((M, 2), dtype=np.float32)
    if out.shape != (M, 2) or out.dtype != np.float32 or (out.size and out.strides[1] != 4):
        raise ValueError("out must be a float32 [M, 2] array with unit column stride")
    if M and (poses.strides[0] % 4 or out.strides[0] % 4 or poses.strides[0] < 0 or out.strides[0] < 0):
        raise ValueError("poses and out rows must be a whole, non-negative number of floats apart")
    if row_speed is not None:
        row_speed = np.ascontiguousarray(row_speed, dtype=np.float64)
    if row_mask is not None:
        row_mask = np.ascontiguousarray(row_mask, dtype=np.uint8)
    for name, t in (("row_speed", row_speed), ("row_mask", row_mask)):
        if t is not None and t.shape != (M,):
            raise ValueError(f"{name} must have shape [M]")
    aux = np.empty((M, 4), dtype=np.float64) if return_aux else None
    p = pursuit_params(**params)
    _lib.check(_lib.load().f110_host_pure_pursuit(track.handle, ctypes.byref(p), ptr(poses), M,
                                                  poses.strides[0] // 4 if M > 1 else poses.shape[1], ptr(row_speed),
                                                  ptr(row_mask), ptr(out), out.strides[0] // 4 if M > 1 else 2,
                                                  ptr(aux)),
               "f110_host_pure_pursuit")
    return (out, aux) if return_aux else out


# ---------------------------------------------------------------- self-play --


def agent_obs(scans: torch.Tensor, obs: torch.Tensor, agent: int, lidar_max: float, out: torch.Tensor | None = None):
    """The flat observation as agent ``agent`` sees it (f110_agent_obs): its scan
    normalised as the step normalises the ego's, its pose group, then the other
    agents' pose groups in ascending index.  scans: float32 device tensor
    [E, A, B] (``sim.out.scans``); obs: the step's float32 obs [E, >= B + 4A]
    (rows may be strided; only the pose block is read); out: float32
    [E, >= B + 4A] (rows may be strided; a new packed tensor if None), which is
    returned.  agent == the step's ego reproduces obs[:, :B + 4A] bit for bit."""
    if scans.dim() != 3 or scans.dtype != torch.float32 or scans.device.type != "cuda" or not scans.is_contiguous():
        raise ValueError("scans must be a contiguous float32 cuda tensor [E, A, B]")
    E, A, B = scans.shape
    W = B + 4 * A
    if out is None:
        out = torch.empty(E, W, dtype=torch.float32, device=scans.device)
    for name, t in (("obs", obs), ("out", out)):
        if (t.dim() != 2 or t.dtype != torch.float32 or t.device != scans.device or t.shape[0] != E or t.shape[1] < W
                or t.stride(1) != 1 or (E > 1 and t.stride(0) < W)):
            raise ValueError(f"{name} must be a float32 [E, >= B + 4A] tensor on the scans' device, unit column stride")
    if not 0 <= int(agent) < A:
        raise ValueError(f"agent must be in [0, {A}); got {agent}")
    _lib.check(_lib.load().f110_agent_obs(ptr(scans), A * B, ptr(obs), row_stride(obs), E, A, B, int(agent),
                                          float(lidar_max), ptr(out), row_stride(out), current_stream(scans.device)),
               "f110_agent_obs")
    return out


def host_agent_obs(scans: np.ndarray, obs: np.ndarray, agent: int, lidar_max: float, out: np.ndarray | None = None):
    """f110_host_agent_obs over NumPy arrays (scans [E, A, B], obs / out [E, >= B + 4A] float32,
    C-contiguous): the host statement of agent_obs, for tests without a GPU."""
    scans = np.ascontiguousarray(scans, dtype=np.float32)
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    E, A, B = scans.shape
    if out is None:
        out = np.empty((E, B + 4 * A), dtype=np.float32)
    if out.dtype != np.float32 or not out.flags.c_contiguous or out.ndim != 2 or obs.ndim != 2:
        raise ValueError("obs and out must be C-contiguous float32 [E, >= B + 4A] arrays")
    _lib.check(_lib.load().f110_host_agent_obs(scans.ctypes.data, A * B, obs.ctypes.data, obs.shape[1], E, A, B,
                                               int(agent), float(lidar_max), out.ctypes.data, out.shape[1]),
               "f110_host_agent_obs")
    return out


def policy_head_rows(h: torch.Tensor, W: torch.Tensor, b: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                     out: torch.Tensor, row_mask: torch.Tensor | None = None):
    """scale * tanh(h W^T + b) + shift (f110_policy_head_rows; the actor head without noise) into
    the rows of ``out`` ([M, nout] float32, rows may be strided, e.g. ``act[:, 1]`` of an [M, A, 2]
    action buffer) with row_mask != 0 (uint8 [M]; None: every row).  The other rows keep their values."""
    M, K = h.shape
    n = W.shape[0]
    if h.dtype != torch.float32 or not h.is_contiguous() or not W.is_contiguous() or W.shape[1] != K:
        raise ValueError("policy_head_rows: h [M, K] and W [nout, K] must be contiguous float32")
    if out.shape != (M, n) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != h.device:
        raise ValueError("policy_head_rows: out must be [M, nout] float32 on h's device with unit column stride")
    if row_mask is not None and (row_mask.dtype != torch.uint8 or row_mask.shape != (M,) or not row_mask.is_contiguous()
                                 or row_mask.device != h.device):
        raise ValueError("policy_head_rows: row_mask must be a contiguous uint8 [M] tensor on h's device")
    _lib.check(_lib.load().f110_policy_head_rows(ptr(h), ptr(W), ptr(b), ptr(scale), ptr(shift), M, K, n,
                                                 ptr(row_mask), ptr(out), row_stride(out), current_stream(h.device)),
               "f110_policy_head_rows")
    return out


def selfplay_mask(n: int, env_offset: int = 0, fraction: float = 1.0) -> np.ndarray:
    """uint8 [n]: 1 where env ``g = env_offset + e`` races the policy opponent, 0 where it races
    gap_follow.  Fixed per global env id, so neither the sharding nor the GPU count changes it:
    ``((g * 2654435761) mod 2^32) < fraction * 2^32`` (Knuth's multiplicative hash of the id)."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"fraction must be in [0, 1]; got {fraction!r}")
    g = np.arange(int(env_offset), int(env_offset) + int(n), dtype=np.uint64)
    hashed = (g * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (hashed.astype(np.float64) < float(fraction) * 4294967296.0).astype(np.uint8)


class PolicyOpponent:
    """A frozen copy of a ddpg.Actor that drives the opponent car on the device.

    The copy's parameters live in one flat buffer (``flat``) allocated here once, and its
    observations in one fixed [n_envs, obs_dim] buffer (``obs``), so a captured step graph that
    holds ``act``'s launches sees new weights after a ``load`` without a re-capture.  The action
    bounds are the source actor's at construction.  Device only: a device or actor shape the
    explicit learner path does not take (learner_fused.ExplicitUpdate.actor_supported) is a
    ValueError -- there is no torch path to keep in step.

    ``track_obs``: a track_obs.TrackObs built for the opponent's seat (``seat=opponent_idx,
    other=ego_idx``) when the actor takes the track observation after the ``B + 4A`` columns
    (obs_dim = B + 4A + width); ``act`` then fills the tail of ``obs`` after agent_obs.  It needs
    the env's simulator, so a trainer that builds the snapshot first hands it over with
    ``set_track_obs`` once the env exists.

    ``scan_obs``: a scan_obs.ScanObs of this snapshot's own (its own ring) when the actor takes the
    compact observation (obs_dim = its width): ``act`` then builds the seat's full row (agent_obs,
    then the track tail, if any) in a buffer of its own and pushes it into ``obs``, refilling the
    rows the simulator's ``was_reset`` flags mark.  F110VectorEnv.reset empties the ring.  With both,
    hand over the scan observation first: the track block's width is then checked against its full
    row."""

    def __init__(self, actor, n_envs: int, device, lidar_max: float = 30.0, track_obs=None, scan_obs=None):
        from .ddpg import Actor, flatten_params
        from .learner_fused import ExplicitUpdate
        self.device = as_device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not ExplicitUpdate.actor_supported(actor, self.device):
            raise ValueError("PolicyOpponent needs a HIP device and an actor of the explicit learner path "
                             "(hidden width 128, act_dim <= 2)")
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError(f"n_envs must be at least 1; got {n_envs}")
        self.lidar_max = float(lidar_max)
        self.obs_dim, self.act_dim = actor.fc1.in_features, actor.fc3.out_features
        low, high = actor.action_low.detach().cpu().tolist(), actor.action_high.detach().cpu().tolist()
        with torch.random.fork_rng(devices=[]):  # the copy's throw-away init draws leave the caller's generator alone
            self.actor = Actor(self.obs_dim, self.act_dim, low, high)
        self.actor = self.actor.to(self.device).requires_grad_(False)
        self.flat = flatten_params(self.actor)
        self._scale, self._shift = (t.contiguous() for t in self.actor._affine())
        self.obs = torch.zeros(self.n_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        self.track_obs = self.scan_obs = self._full = None
        if scan_obs is not None:
            self.set_scan_obs(scan_obs)
        if track_obs is not None:
            self.set_track_obs(track_obs)
        self.load(actor)

    def set_track_obs(self, track_obs):
        """The TrackObs whose block follows the ``B + 4A`` columns of this actor's (full) observation."""
        sim = track_obs.sim
        full = self.obs_dim if self.scan_obs is None else self.scan_obs.in_width
        if sim.E != self.n_envs or sim.device != self.device or sim.B + 4 * sim.A + track_obs.width != full:
            raise ValueError(f"PolicyOpponent: the track observation must be built for {self.n_envs} envs on "
                             f"{self.device} and fill the actor's {full} columns after B + 4A")
        self.track_obs = track_obs

    def set_scan_obs(self, scan_obs):
        """The ScanObs that makes this actor's compact observation from the seat's full row."""
        if scan_obs.n_envs != self.n_envs or scan_obs.device != self.device or scan_obs.width != self.obs_dim:
            raise ValueError(f"PolicyOpponent: the scan observation must be built for {self.n_envs} envs on "
                             f"{self.device} and give the actor's {self.obs_dim} columns; it gives {scan_obs.width}")
        self.scan_obs = scan_obs
        self._full = torch.zeros(self.n_envs, scan_obs.in_width, dtype=torch.float32, device=self.device)

    @staticmethod
    def _flat_of(actor):
        """The flat buffer an actor's parameters are views of, in parameter order (flatten_params'
        layout), or None."""
        params = list(actor.parameters())
        p0, off = params[0], 0
        for p in params:
            if (not p.is_contiguous() or p.untyped_storage().data_ptr() != p0.untyped_storage().data_ptr()
                    or p.storage_offset() != p0.storage_offset() + off):
                return None
            off += p.numel()
        return torch.empty(0, dtype=p0.dtype, device=p0.device).set_(p0.untyped_storage(), p0.storage_offset(), (off,))

    def load(self, actor):
        """Take ``actor``'s weights: one flat device-to-device copy on the current stream when its
        parameters are one flat buffer (a learner's on the GPU are), else one copy per parameter."""
        src = [p.detach() for p in actor.parameters()]
        dst = list(self.actor.parameters())
        if len(src) != len(dst) or any(a.shape != b.shape for a, b in zip(src, dst)):
            raise ValueError("PolicyOpponent.load: the actor's shape differs from the snapshot's")
        flat = self._flat_of(actor) if src[0].device == self.device and src[0].dtype == torch.float32 else None
        with torch.no_grad():
            if flat is not None:
                self.flat.copy_(flat)
            else:
                for a, b in zip(src, dst):
                    b.copy_(a)

    def state_dict(self):
        return self.actor.state_dict()

    def load_state_dict(self, sd):
        """The parameters of a saved snapshot, copied into the flat buffer in place."""
        with torch.no_grad():
            for name, p in self.actor.named_parameters():
                p.copy_(sd[name])

    def act(self, sim_out, agent: int, out_rows: torch.Tensor, row_mask: torch.Tensor | None = None, obs=None):
        """The snapshot's action (no noise: choose_action(training=False)) for agent ``agent`` of
        every env, from the simulator outputs ``sim_out`` (obs: the step's obs tensor when the step
        wrote it elsewhere than sim_out.obs), into ``out_rows`` ([n_envs, act_dim] float32, rows may
        be strided) where row_mask != 0 (None: every row).  Three stages on the current stream:
        f110_agent_obs into the fixed buffer (then the track observation's tail, if any, and with a
        scan observation its push from the full row into the fixed compact buffer), fc1 and fc2 on
        the learner GEMMs over all rows, f110_policy_head_rows."""
        from .learner_fused import ExplicitUpdate
        full = self.obs if self.scan_obs is None else self._full  # the seat's full row
        agent_obs(sim_out.scans, sim_out.obs if obs is None else obs, agent, self.lidar_max, out=full)
        head = sim_out.scans.shape[2] + 4 * sim_out.scans.shape[1]
        if self.track_obs is not None:
            self.track_obs.fill(full[:, head:])
        elif full.shape[1] != head:  # (no quiet zeros for columns the actor was trained on)
            raise ValueError(f"PolicyOpponent: the actor takes {full.shape[1]} columns, the step gives {head}: "
                             "set_track_obs is missing")
        if self.scan_obs is not None:
            self.scan_obs.push(full, reset=sim_out.was_reset, out=self.obs)
        h2 = ExplicitUpdate.actor_hidden(self.actor, self.obs)
        return policy_head_rows(h2, self.actor.fc3.weight, self.actor.fc3.bias, self._scale, self._shift, out_rows,
                                row_mask)
