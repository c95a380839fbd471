"""The sensor randomization on the device (include/f110.h, "sensor randomization").

No reference counterpart: the reference's scan noise is one std for every env, no beam ever drops
out and the poses are exact.  This stage turns a full row ``[B ranges | M middle (pose) columns | T
tail (track) columns]`` into the row a policy sees through an imperfect sensor: the ranges scaled,
noised, quantized, dropped and blacked out, the pose columns noised, under parameters drawn per env
and episode from ``(lo, hi)`` ranges, keyed by (seed, global env id).  The collision columns and the
tail are carried through; the default ranges are the identity.

``SensorModel`` owns the per-env parameter rows and counters and applies the rule in one launch on
the current stream (f110_sensor_apply: capturable, the counters live on the device),
``host_sensor_apply`` is its host statement over NumPy arrays (same bits, no GPU).
F110VectorEnv(sensor_ranges=...) uses ``SensorModel``; every other consumer of the observation keeps
reading the clean rows.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._dev import cuda_device, f32_rows, ptr, u8_rows
from ._dev import stream as current_stream

SENSOR_FIELDS = tuple(n for n, _ in _lib.F110SensorParams._fields_)  # scale, noise_abs, ..., pose_theta
PARAM_ROW = ("scale", "noise_abs_n", "noise_rel", "dropout", "blackout_width", "blackout_start", "quant_n",
             "pose_xy", "pose_theta", "dropout_threshold")  # f110_sensor_arrays' parameter row
MAX_BEAMS = 4096  # csrc/f110_sensor.h


def sensor_ranges(n_beams: int | None = None, **ranges) -> "_lib.F110SensorParams":
    """f110_default_sensor_params (the identity) with ``ranges`` on top: each of scale, noise_abs,
    noise_rel, dropout, blackout, quant, pose_xy, pose_theta a ``(lo, hi)`` pair or one number (lo =
    hi).  An unknown name, a value that is no pair of finite numbers, lo > hi or a value out of range
    is a ValueError; ``n_beams`` (default: the limit, 4096) bounds blackout."""
    p = _lib.F110SensorParams()
    L = _lib.load()
    L.f110_default_sensor_params(ctypes.byref(p))
    for k, v in ranges.items():
        if k not in SENSOR_FIELDS:
            raise ValueError(f"unknown sensor parameter {k!r} (known: {', '.join(SENSOR_FIELDS)})")
        try:
            if isinstance(v, (bool, str)):
                raise TypeError
            lo, hi = (float(v), float(v)) if isinstance(v, (int, float, np.integer, np.floating)) else map(float, v)
        except (TypeError, ValueError):
            raise ValueError(f"sensor randomization: {k} takes (lo, hi) or one number; got {v!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"sensor randomization: {k} must be finite; got {v!r}")
        getattr(p, k)[0], getattr(p, k)[1] = lo, hi
    B = MAX_BEAMS if n_beams is None else int(n_beams)
    if L.f110_host_check_sensor_params(ctypes.byref(p), B) != 0:
        raise ValueError("sensor randomization: " + L.f110_last_error().decode().split(": ", 1)[-1])
    return p


def _shape(n_envs, n_beams, n_mid, n_tail, range_max, env_offset):
    N, B, M, T = int(n_envs), int(n_beams), int(n_mid), int(n_tail)
    if N < 1 or not 1 <= B <= MAX_BEAMS or M < 0 or M % 4 or T < 0:
        raise ValueError(f"sensor randomization: n_envs >= 1, n_beams in [1, {MAX_BEAMS}], n_mid a multiple of 4 and "
                         f"n_tail >= 0; got {n_envs}, {n_beams}, {n_mid}, {n_tail}")
    if not (float(range_max) > 0.0 and math.isfinite(float(range_max))):
        raise ValueError(f"sensor randomization: range_max must be > 0; got {range_max!r}")
    if int(env_offset) < 0:
        raise ValueError(f"sensor randomization: env_offset must be >= 0; got {env_offset!r}")
    return N, B, M, T


def _mask(mask, n):
    """The env mask as a contiguous host uint8 [n] array (None stays None)."""
    if mask is None:
        return None
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    m = np.asarray(mask)
    if m.shape != (n,) or m.dtype.kind not in "bui":
        raise ValueError(f"sensor randomization: the env mask must be a uint8 / bool [{n}] array")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def host_sensor_state(n_envs: int) -> dict:
    """A fresh host state in f110_sensor_arrays' layout: params [N, 10] float32 zeros, episode [N]
    int32 of -1 (no apply yet), step [N] int32 zeros."""
    N = int(n_envs)
    return {"params": np.zeros((N, len(PARAM_ROW)), np.float32), "episode": np.full(N, -1, np.int32),
            "step": np.zeros(N, np.int32)}


def _np_stride(a, n, width, what):
    if (not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != (n, width)
            or (a.size and a.strides[1] != 4)):
        raise ValueError(f"{what} must be a float32 [{n}, {width}] array with unit column stride")
    if n > 1 and (a.strides[0] % 4 or a.strides[0] < 4 * width):
        raise ValueError(f"{what}: rows must be a whole number of floats apart, at least the width")
    return a.strides[0] // 4 if n > 1 else width


def host_sensor_apply(state: dict, rows: np.ndarray, n_beams: int, n_mid: int, n_tail: int = 0, range_max: float = 30.0,
                      seed: int = 0, env_offset: int = 0, mask=None, reset=None, out: np.ndarray | None = None, **ranges):
    """One apply on the host (f110_host_sensor_apply) over NumPy arrays; ``state`` as
    host_sensor_state makes it, updated in place.  rows and out: float32 [N, B + M + T], either may
    have strided rows; out may be rows itself (in place), a new array if None.  mask: uint8 / bool
    [N] or None (every env is touched); reset: uint8 / bool [N] or None.  Returns out."""
    par, ep, st = state["params"], state["episode"], state["step"]
    N = ep.shape[0]
    N, B, M, T = _shape(N, n_beams, n_mid, n_tail, range_max, env_offset)
    p = sensor_ranges(B, **ranges)
    if (par.dtype != np.float32 or ep.dtype != np.int32 or st.dtype != np.int32 or par.shape != (N, len(PARAM_ROW))
            or st.shape != (N,) or not (par.flags.c_contiguous and ep.flags.c_contiguous and st.flags.c_contiguous)):
        raise ValueError("state must come from host_sensor_state")
    W = B + M + T
    rs = _np_stride(rows, N, W, "rows")
    if out is None:
        out = np.empty((N, W), dtype=np.float32)
    os_ = _np_stride(out, N, W, "out")
    m = _mask(mask, N)
    if reset is not None:
        reset = np.ascontiguousarray(np.asarray(reset).astype(np.uint8).reshape(-1))
        if reset.shape[0] != N:
            raise ValueError(f"reset must have {N} entries; got {reset.shape[0]}")
    try:
        _lib.check(_lib.load().f110_host_sensor_apply(
            ctypes.byref(p), N, B, M, T, float(range_max), int(seed), int(env_offset), ptr(m), rows.ctypes.data, rs,
            ptr(reset), par.ctypes.data, ep.ctypes.data, st.ctypes.data, out.ctypes.data, os_), "f110_host_sensor_apply")
    except _lib.F110Error as exc:  # (every refusal of this entry is a bad argument)
        raise ValueError(str(exc)) from exc
    return out


class SensorModel:
    """The sensor randomization of ``n_envs`` envs: the library's parameter rows and counters on
    ``device`` and one launch per ``apply`` on the current stream.  ``mask`` (uint8 / bool [n_envs],
    fixed at creation): the envs the stage touches; an env with 0 is copied through (its counters
    still advance).  ranges: see sensor_ranges."""

    def __init__(self, n_envs: int, n_beams: int, n_mid: int, n_tail: int = 0, range_max: float = 30.0, seed: int = 0,
                 env_offset: int = 0, mask=None, device=0, **ranges):
        self.handle = None
        self.n_envs, self.n_beams, self.n_mid, self.n_tail = _shape(n_envs, n_beams, n_mid, n_tail, range_max,
                                                                    env_offset)
        self.params = sensor_ranges(self.n_beams, **ranges)
        self.width = self.n_beams + self.n_mid + self.n_tail
        self.range_max, self.seed, self.env_offset = float(range_max), int(seed), int(env_offset)
        self.mask = _mask(mask, self.n_envs)
        self.device = dev = cuda_device(device, "SensorModel")
        if dev.index is None:
            self.device = dev = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self.L.f110_sensor_create(ctypes.byref(h), dev.index, self.n_envs, self.n_beams, self.n_mid,
                                             self.n_tail, self.range_max, self.seed & (2 ** 64 - 1), self.env_offset,
                                             ptr(self.mask), ctypes.byref(self.params)), "f110_sensor_create")
        self.handle = h
        self._keep = None  # a call's converted flags, alive until the stream has consumed them

    def apply(self, rows: torch.Tensor, reset=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """rows: float32 [n_envs, B + M + T] on the device (unit column stride, rows may be strided);
        reset: uint8 / bool [n_envs] or None: the envs whose episode starts with this row (an env's
        first apply does anyway); out: float32 [n_envs, B + M + T], rows itself (in place) or
        disjoint from it, a new tensor if None.  Returns out."""
        rs = f32_rows(rows, self.n_envs, self.width, self.device, "SensorModel.apply: rows", copy_ok=False)[1]
        if out is None:
            out = torch.empty(self.n_envs, self.width, dtype=torch.float32, device=self.device)
        os_ = f32_rows(out, self.n_envs, self.width, self.device, "SensorModel.apply: out", copy_ok=False)[1]
        self._keep = m = u8_rows(reset, self.n_envs, self.device, "reset")
        rc = self.L.f110_sensor_apply(self.handle, ptr(rows), rs, ptr(m), ptr(out), os_, current_stream(self.device))
        if rc == -1:  # F110_E_INVALID
            raise ValueError(self.L.f110_last_error().decode())
        _lib.check(rc, "f110_sensor_apply")
        return out

    def reset(self, mask=None):
        """Restart the counters of the envs with mask != 0 (None: all): their next apply starts
        episode 0 again and redraws their parameters."""
        self._keep = m = u8_rows(mask, self.n_envs, self.device, "mask")
        _lib.check(self.L.f110_sensor_reset(self.handle, ptr(m), current_stream(self.device)), "f110_sensor_reset")

    def arrays(self) -> dict:
        """Device copies of the state: params [N, 10] float32 (PARAM_ROW names the columns), episode
        and step [N] int32."""
        from .replay import _d2d
        par, ep, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.L.f110_sensor_arrays(self.handle, ctypes.byref(par), ctypes.byref(ep), ctypes.byref(st)),
                   "f110_sensor_arrays")
        out = {"params": torch.empty(self.n_envs, len(PARAM_ROW), dtype=torch.float32, device=self.device),
               "episode": torch.empty(self.n_envs, dtype=torch.int32, device=self.device),
               "step": torch.empty(self.n_envs, dtype=torch.int32, device=self.device)}
        for k, src in (("params", par), ("episode", ep), ("step", st)):
            _d2d(out[k], src.value, current_stream(self.device))
        return out

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.L.f110_sensor_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
