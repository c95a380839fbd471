"""The track-relative observation block on the device (include/f110.h, "track observation").

No reference counterpart: the reference's flat observation stops at the scaled ranges and each
car's (x, y, yaw, collision) in map coordinates.  This block adds, per env, the seat car's own
dynamic state (speed, steering angle, yaw rate, slip), its lateral offset and heading error on a
CenterlineTrack, a preview of the centerline ahead in the car's frame and the other car's gap,
as ``width`` float32 columns (a multiple of 4) meant to follow the step's ``B + 4A`` columns.

``track_obs`` runs f110_track_obs on any SoA state ([7, E*A] float64, BatchSim.get_state's layout),
``host_track_obs`` is its host statement over NumPy arrays (same bits), and ``TrackObs`` binds a
BatchSim's live state to a track and fills the tail of an observation buffer in one launch
(f110_ctx_track_obs): F110VectorEnv(track_obs=True) and PolicyOpponent(track_obs=...) use it.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._dev import device_track, f32_rows, ptr
from ._dev import stream as current_stream

TRACK_OBS_FIELDS = ("v_scale", "steer_scale", "yaw_rate_scale", "slip_scale", "lat_scale", "gap_scale", "preview",
                    "direction")
MAX_PREVIEW = 8
OWN_COLUMNS = 7  # v, delta, yaw_rate, slip, t, sin and cos of the heading error


def track_obs_params(**params) -> "_lib.F110TrackObsParams":
    """f110_default_track_obs_params with ``params`` (v_scale, steer_scale, yaw_rate_scale,
    slip_scale, lat_scale, gap_scale, preview, direction) on top; an unknown name is a ValueError.
    ``preview`` is a sequence of 0..8 distances in metres (it sets n_preview).  The values
    themselves are checked by the library at the call."""
    p = _lib.F110TrackObsParams()
    _lib.load().f110_default_track_obs_params(ctypes.byref(p))
    for k, v in params.items():
        if k not in TRACK_OBS_FIELDS:
            raise ValueError(f"unknown track-observation parameter {k!r} (known: {', '.join(TRACK_OBS_FIELDS)})")
        if k == "direction":
            if v not in (1, -1):
                raise ValueError(f"direction must be +1 or -1; got {v!r}")
            p.direction = int(v)
        elif k == "preview":
            d = [float(x) for x in v]
            if len(d) > MAX_PREVIEW:
                raise ValueError(f"preview takes at most {MAX_PREVIEW} distances; got {len(d)}")
            p.n_preview = len(d)
            for j in range(MAX_PREVIEW):
                p.preview[j] = d[j] if j < len(d) else 0.0
        else:
            setattr(p, k, float(v))
    return p


def track_obs_width(n_preview: int = 4, has_other: bool = False) -> int:
    """f110_track_obs_width: 7 + 2*n_preview + (3 with another car), rounded up to a multiple of 4."""
    w = _lib.load().f110_track_obs_width(int(n_preview), int(bool(has_other)))
    if w < 0:
        raise ValueError(f"n_preview must be in [0, {MAX_PREVIEW}]; got {n_preview}")
    return int(w)


def track_obs_columns(n_preview: int = 4, has_other: bool = False):
    """(low, high) float32 [width]: [-1, 1] for the two heading-error columns and the gap column,
    +-inf for the rest (the pad columns are 0 but unbounded here)."""
    w = track_obs_width(n_preview, has_other)
    low, high = np.full(w, -np.inf, np.float32), np.full(w, np.inf, np.float32)
    unit = [5, 6] + ([OWN_COLUMNS + 2 * int(n_preview)] if has_other else [])
    low[unit], high[unit] = -1.0, 1.0
    return low, high


def _seats(n_agents, seat, other, what):
    seat, other = int(seat), -1 if other is None else int(other)
    if not 1 <= int(n_agents) <= 8:
        raise ValueError(f"{what}: n_agents must be in [1, 8]; got {n_agents}")
    if not 0 <= seat < n_agents:
        raise ValueError(f"{what}: seat must be in [0, {n_agents}); got {seat}")
    if other != -1 and (not 0 <= other < n_agents or other == seat):
        raise ValueError(f"{what}: other must be None or another agent in [0, {n_agents}); got {other}")
    return seat, other


def track_obs(state: torch.Tensor, track, n_envs: int, n_agents: int, seat: int = 0, other=None,
              out: torch.Tensor | None = None, stream=None, **params):
    """The block for ``n_envs`` envs (f110_track_obs).  state: float64 device tensor [7, n_envs *
    n_agents] (BatchSim.get_state()[0]); track: a device reward.CenterlineTrack; seat: the car the
    block is about, other: the car its gap columns are about (None: no gap columns).  Returns out
    [n_envs, width] float32, written into ``out`` if given (rows may be strided, e.g. the tail
    ``obs[:, B + 4A:]`` of a wide obs buffer); params: see track_obs_params."""
    E, A = int(n_envs), int(n_agents)
    seat, other = _seats(A, seat, other, "track_obs")
    if (state.dtype != torch.float64 or state.device.type != "cuda" or tuple(state.shape) != (7, E * A)
            or not state.is_contiguous()):
        raise ValueError(f"state must be a contiguous float64 cuda tensor [7, {E * A}]")
    device_track(track, state.device, "track", user="the state")
    p = track_obs_params(**params)
    width = track_obs_width(p.n_preview, other >= 0)
    if out is None:
        out = torch.empty(E, width, dtype=torch.float32, device=state.device)
    stride = f32_rows(out, E, width, state.device, "track_obs: out", copy_ok=False)[1]
    _lib.check(_lib.load().f110_track_obs(track.handle, ctypes.byref(p), ptr(state), E, A, seat, other, ptr(out),
                                          stride, current_stream(state.device, stream)), "f110_track_obs")
    return out


def host_track_obs(state: np.ndarray, track, n_envs: int, n_agents: int, seat: int = 0, other=None,
                   out: np.ndarray | None = None, **params):
    """f110_host_track_obs over NumPy arrays: the host statement of track_obs, for tests without a
    GPU (track: any CenterlineTrack, ``device=None`` included).  state: float64 [7, n_envs *
    n_agents]; out: float32 [n_envs, width], rows may be strided (unit stride inside a row)."""
    E, A = int(n_envs), int(n_agents)
    seat, other = _seats(A, seat, other, "host_track_obs")
    state = np.ascontiguousarray(state, dtype=np.float64)
    if state.shape != (7, E * A):
        raise ValueError(f"state must be a float64 array [7, {E * A}]")
    if not getattr(track, "handle", None):
        raise ValueError("track must be an open reward.CenterlineTrack")
    p = track_obs_params(**params)
    width = track_obs_width(p.n_preview, other >= 0)
    if out is None:
        out = np.empty((E, width), dtype=np.float32)
    if out.shape != (E, width) or out.dtype != np.float32 or (out.size and out.strides[1] != 4):
        raise ValueError(f"out must be a float32 [{E}, {width}] array with unit column stride")
    if E > 1 and (out.strides[0] % 4 or out.strides[0] < 4 * width):
        raise ValueError("out rows must be a whole number of floats apart, at least width")
    _lib.check(_lib.load().f110_host_track_obs(track.handle, ctypes.byref(p), state.ctypes.data, E, A, seat, other,
                                               out.ctypes.data, out.strides[0] // 4 if E > 1 else width),
               "f110_host_track_obs")
    return out


class TrackObs:
    """The block of one seat of a BatchSim on one track: ``fill`` writes it for every env from the
    simulator's live state (f110_ctx_track_obs: no copy of the state, one launch on the current
    stream, capturable).  ``width`` is the number of columns; ``low`` / ``high`` their bounds."""

    def __init__(self, sim, track, seat: int = 0, other=None, **params):
        self.sim, self.track = sim, track
        self.seat, self.other = _seats(sim.A, seat, other, "TrackObs")
        device_track(track, sim.device, "the track", "TrackObs needs an open device reward.CenterlineTrack",
                     user="the simulator")
        self.params = track_obs_params(**params)
        if any(not 0.0 < self.params.preview[j] < track.L for j in range(self.params.n_preview)):
            raise ValueError(f"preview distances must be in (0, {track.L}) m")
        self.n_preview = int(self.params.n_preview)
        self.width = track_obs_width(self.n_preview, self.other >= 0)
        self.low, self.high = track_obs_columns(self.n_preview, self.other >= 0)

    def fill(self, out_rows: torch.Tensor) -> torch.Tensor:
        """out_rows: float32 [E, width] (unit column stride, rows may be strided), e.g. the tail of
        a wide obs buffer.  Returns it."""
        sim = self.sim
        stride = f32_rows(out_rows, sim.E, self.width, sim.device, "TrackObs.fill: out", copy_ok=False)[1]
        _lib.check(_lib.load().f110_ctx_track_obs(sim.ctx, self.track.handle, ctypes.byref(self.params), self.seat,
                                                  self.other, ptr(out_rows), stride, current_stream(sim.device)),
                   "f110_ctx_track_obs")
        return out_rows
