"""RaceStats: per-env race outcomes and running totals on the device.

Thin owner of the buffers f110_race_stats (include/f110.h, "race statistics") works on: one call
per vector step, on that step's observations and flags, three small launches on the current torch
stream with no host work -- a captured step graph replays it.  Where EpisodeStats answers "what
was the return", this answers "how far did the car get, did it finish ahead of the opponent, how
often did it pass or get passed, and how did the episode end".
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._dev import cuda_device, device_track, f32_rows, ptr as P, stream, u8_rows


def race_params(pass_margin=None, direction: int = 1) -> "_lib.F110RaceParams":
    """f110_default_race_params with the given fields (pass_margin None: the car's length)."""
    p = _lib.F110RaceParams()
    _lib.load().f110_default_race_params(ctypes.byref(p))
    if pass_margin is not None:
        p.pass_margin = float(pass_margin)
    p.direction = int(direction)
    return p


class RaceStats:
    """Race bookkeeping of ``n_envs`` autoresetting envs on ``track`` (a device
    reward.CenterlineTrack).  ``ego_idx`` / ``opponent_idx`` name the pose groups of the flat
    observation ([n_beams scan entries, (x, y, yaw, collision) per agent]); ``opponent_idx=None``
    is a single-agent env: lead, passes and passed stay 0.

    ``begin(obs)`` starts every env's episode at ``obs`` (what an env's ``reset()`` returns);
    ``update(obs, terminated, truncated, was_reset)`` adds one step: a reset row (NEXT_STEP
    autoreset's reset observation) starts a new episode, a row whose ``terminated`` or
    ``truncated`` is set finishes it (terminated wins).  ``progress`` / ``lead`` hold each env's
    running episode, ``last_progress`` / ``last_lead`` / ``last_length`` its last finished one,
    ``result`` the last update's result byte (_lib.RACE_RESULT) and ``finished`` its bit 0;
    ``totals()`` the running totals over all finished episodes."""

    def __init__(self, n_envs: int, track, n_beams: int, ego_idx: int = 0, opponent_idx: int | None = 1,
                 pass_margin: float | None = None, direction: int = 1, device=0):
        self.L = _lib.load()
        dev = cuda_device(device, "RaceStats")
        device_track(track, dev, "the track", "RaceStats needs a device reward.CenterlineTrack", user="RaceStats")
        if opponent_idx is not None and int(opponent_idx) == int(ego_idx):
            raise ValueError("RaceStats: opponent_idx must differ from ego_idx")
        if int(n_beams) < 0 or int(ego_idx) < 0 or (opponent_idx is not None and int(opponent_idx) < 0):
            raise ValueError("RaceStats: n_beams, ego_idx and opponent_idx must be >= 0")
        self.device = dev
        self.track = track
        self.n_envs = n = int(n_envs)
        self.n_beams = int(n_beams)
        self.ego_idx = int(ego_idx)
        self.opponent_idx = None if opponent_idx is None else int(opponent_idx)
        self.params = race_params(pass_margin, direction)
        self.state = torch.zeros(n, _lib.RACE_STATE_BYTES, dtype=torch.uint8, device=dev)
        self._cur = torch.zeros(n, 2, dtype=torch.float64, device=dev)
        self.last_progress = torch.zeros(n, dtype=torch.float64, device=dev)
        self.last_lead = torch.zeros(n, dtype=torch.float64, device=dev)
        self.last_length = torch.zeros(n, dtype=torch.int32, device=dev)
        self.result = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._totals = torch.zeros(_lib.RACE_TOTALS_BYTES, dtype=torch.uint8, device=dev)
        self._scratch = torch.zeros(int(self.L.f110_race_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        self._zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._ones = torch.ones(n, dtype=torch.uint8, device=dev)

    @property
    def progress(self):
        """The running episode's signed progress of the ego, m ([n] float64 view)."""
        return self._cur[:, 0]

    @property
    def lead(self):
        """The running episode's lead over the opponent, m ([n] float64 view; 0 without one)."""
        return self._cur[:, 1]

    @property
    def finished(self):
        """The envs that finished in the last update ([n] bool)."""
        return (self.result & 1).bool()

    def reset(self):
        """Every env is fresh (not started); the per-env outputs are zeroed.  The totals stay."""
        for t in (self.state, self._cur, self.last_progress, self.last_lead, self.last_length, self.result):
            t.zero_()

    def begin(self, obs):
        """Every env's episode starts at ``obs``: one call with every was_reset set."""
        self.update(obs, self._zeros, None, self._ones)

    def update(self, obs, terminated, truncated, was_reset):
        """One step's rows (device tensors: obs float32 [n, obs_len], any row range of a larger
        buffer -- the row stride is the tensor's; flags u8 / bool [n]; truncated may be None).
        Asynchronous on the current stream."""
        n = self.n_envs
        o, stride = f32_rows(obs, n, None, self.device, "RaceStats: obs")
        need = self.n_beams + 4 * (max(self.ego_idx, self.opponent_idx or 0) + 1)
        if o.shape[1] < need:
            raise ValueError(f"RaceStats: obs must be [{n}, >= {need}]; got {tuple(o.shape)}")
        te = u8_rows(terminated, n, self.device, "RaceStats: terminated")
        tr = u8_rows(truncated, n, self.device, "RaceStats: truncated")
        wr = u8_rows(was_reset, n, self.device, "RaceStats: was_reset")
        self._keep = (o, te, tr, wr)
        V = ctypes.c_void_p
        base = o.data_ptr()
        ego = V(base + 4 * (self.n_beams + 4 * self.ego_idx))
        opp = None if self.opponent_idx is None else V(base + 4 * (self.n_beams + 4 * self.opponent_idx))
        _lib.check(self.L.f110_race_stats(self.track.handle, ctypes.byref(self.params), ego, opp, stride, P(te), P(tr),
                                          P(wr), n, P(self.state), P(self._cur), P(self.last_progress),
                                          P(self.last_lead), P(self.last_length), P(self.result), P(self._totals),
                                          P(self._scratch), stream(self.device)), "f110_race_stats")

    def totals(self) -> dict:
        """The running totals as Python numbers (the fields of f110_race_totals; progress_min /
        progress_max are None before the first episode), plus progress_mean, lead_mean, length_mean,
        win_rate (= ahead_at_end / episodes) and crash_rate (= ego_crashes / episodes), None at 0
        episodes.  Waits for the current stream."""
        raw = self._totals.cpu().numpy().tobytes()
        return totals_dict(_lib.F110RaceTotals.from_buffer_copy(raw))

    def reset_totals(self):
        self._totals.zero_()


def totals_dict(totals) -> dict:
    """An _lib.F110RaceTotals as RaceStats.totals() reports it."""
    t = totals.as_dict()
    n = t["episodes"]
    if n == 0:
        t["progress_min"] = t["progress_max"] = None
    for mean, total in (("progress_mean", "progress_sum"), ("lead_mean", "lead_sum"), ("length_mean", "length_sum"),
                        ("win_rate", "ahead_at_end"), ("crash_rate", "ego_crashes")):
        t[mean] = t[total] / n if n else None
    return t


def host_race_stats(track, params, ego, opp, terminated, truncated, was_reset, state, cur=None, last_progress=None,
                    last_lead=None, last_length=None, result=None, totals=None):
    """f110_host_race_stats over NumPy arrays (in place): the device's semantics in ascending env
    order.  track: a reward.CenterlineTrack (device=None will do); params: an _lib.F110RaceParams;
    ego / opp: float32 [n, >= 4] pose-group views with a contiguous last axis and the same row
    stride (opp may be None); state: uint8 [n, 64] (f110_race_state rows); totals: an
    _lib.F110RaceTotals."""
    L = _lib.load()
    n = int(ego.shape[0])
    for a in (ego, opp):
        if a is not None and (a.dtype != np.float32 or a.ndim != 2 or a.shape[1] < 4 or a.strides[1] != 4 or
                              a.strides[0] % 4 or a.shape[0] != n):
            raise ValueError("host_race_stats: ego / opp must be float32 [n, >= 4] with a contiguous last axis")
    if opp is not None and n > 1 and opp.strides[0] != ego.strides[0]:
        raise ValueError("host_race_stats: ego and opp must share one row stride")
    for a, dt in ((terminated, np.uint8), (truncated, np.uint8), (was_reset, np.uint8), (state, np.uint8),
                  (cur, np.float64), (last_progress, np.float64), (last_lead, np.float64), (last_length, np.int32),
                  (result, np.uint8)):
        if a is not None and (a.dtype != dt or not a.flags.c_contiguous):
            raise ValueError("host_race_stats: arrays must be C-contiguous float64 / uint8 / int32 as declared")
    stride = ego.strides[0] // 4 if n > 1 else max(ego.strides[0] // 4, 4)
    _lib.check(L.f110_host_race_stats(track.handle, ctypes.byref(params), P(ego), P(opp), stride, P(terminated),
                                      P(truncated), P(was_reset), n, P(state), P(cur), P(last_progress), P(last_lead),
                                      P(last_length), P(result), None if totals is None else ctypes.byref(totals)),
               "f110_host_race_stats")
