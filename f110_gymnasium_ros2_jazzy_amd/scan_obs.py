"""The compact LiDAR observation on the device (include/f110.h, "scan observation").

No reference counterpart: the reference's flat observation hands the policy all 1080 scaled ranges
of one frame.  This stage turns a full row ``[B ranges | M middle (pose) columns | T tail (track)
columns]`` into a compact policy row ``[F*K | M if keep_mid | T]``: the ranges pooled into ``K``
sectors (min or mean), the last ``F`` pooled frames stacked ``S`` pushes apart, newest first, out of
a per-env ring on the device; the other columns are the current row's.

``ScanObs`` owns the ring and pushes rows in one launch on the current stream (f110_scan_obs_push:
capturable, the ring's head lives on the device), ``host_scan_obs_push`` is its host statement over
NumPy arrays (same bits, no GPU).  F110VectorEnv(scan_obs=...) and PolicyOpponent(scan_obs=...) use
``ScanObs``; every other consumer of the observation keeps reading the full rows.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._dev import cuda_device, f32_rows, ptr, u8_rows
from ._dev import stream as current_stream

SCAN_OBS_FIELDS = ("n_bins", "n_frames", "stride", "reduce", "keep_mid")
REDUCES = ("min", "mean")
MAX_FRAMES, MAX_STRIDE, MAX_DEPTH, MAX_BEAMS = 8, 16, 32, 4096  # csrc/f110_scan_obs.h


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"scan observation: {name} must be an integer in [{lo}, {hi}]; got {v!r}")
    return int(v)


def scan_obs_params(n_beams: int | None = None, **params) -> "_lib.F110ScanObsParams":
    """f110_default_scan_obs_params with ``params`` (n_bins, n_frames, stride, reduce = "min" |
    "mean" | 0 | 1, keep_mid) on top.  An unknown name or a value out of range is a ValueError;
    ``n_beams`` (if given) bounds n_bins."""
    p = _lib.F110ScanObsParams()
    _lib.load().f110_default_scan_obs_params(ctypes.byref(p))
    for k, v in params.items():
        if k not in SCAN_OBS_FIELDS:
            raise ValueError(f"unknown scan-observation parameter {k!r} (known: {', '.join(SCAN_OBS_FIELDS)})")
        if k == "reduce":
            if isinstance(v, str):
                if v not in REDUCES:
                    raise ValueError(f"scan observation: reduce must be 'min' or 'mean'; got {v!r}")
                v = REDUCES.index(v)
            p.reduce = _int("reduce", v, 0, 1)
        elif k == "keep_mid":
            p.keep_mid = _int("keep_mid", int(v) if isinstance(v, (bool, np.bool_)) else v, 0, 1)
        elif k == "n_bins":
            p.n_bins = _int("n_bins", v, 1, MAX_BEAMS)
        elif k == "n_frames":
            p.n_frames = _int("n_frames", v, 1, MAX_FRAMES)
        else:
            p.stride = _int("stride", v, 1, MAX_STRIDE)
    if (p.n_frames - 1) * p.stride + 1 > MAX_DEPTH:
        raise ValueError(f"scan observation: the ring depth (n_frames - 1) * stride + 1 must not exceed {MAX_DEPTH}; "
                         f"got {(p.n_frames - 1) * p.stride + 1}")
    if n_beams is not None and p.n_bins > int(n_beams):
        raise ValueError(f"scan observation: n_bins must not exceed the {int(n_beams)} beams; got {p.n_bins}")
    return p


def _shape(n_beams, n_mid, n_tail):
    B, M, T = int(n_beams), int(n_mid), int(n_tail)
    if not 1 <= B <= MAX_BEAMS or M < 0 or T < 0:
        raise ValueError(f"scan observation: n_beams must be in [1, {MAX_BEAMS}], n_mid and n_tail >= 0; "
                         f"got {n_beams}, {n_mid}, {n_tail}")
    return B, M, T


def scan_obs_width(n_beams: int, n_mid: int, n_tail: int = 0, **params) -> int:
    """f110_scan_obs_width: n_frames * n_bins + (n_mid if keep_mid) + n_tail."""
    B, M, T = _shape(n_beams, n_mid, n_tail)
    p = scan_obs_params(B, **params)
    w = _lib.load().f110_scan_obs_width(ctypes.byref(p), B, M, T)
    if w < 0:
        raise ValueError("scan observation: the library refuses these parameters")
    return int(w)


def scan_obs_depth(p) -> int:
    """The ring depth D = (n_frames - 1) * stride + 1."""
    return (int(p.n_frames) - 1) * int(p.stride) + 1


def host_scan_obs_state(n_envs: int, n_beams: int, **params) -> dict:
    """A fresh host ring in f110_scan_obs_arrays' layout: ring [N, D, K] float32 zeros, head [N]
    int32 of -1 (empty)."""
    p = scan_obs_params(int(n_beams), **params)
    return {"ring": np.zeros((int(n_envs), scan_obs_depth(p), int(p.n_bins)), np.float32),
            "head": np.full(int(n_envs), -1, np.int32)}


def _np_stride(a, width, what):
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != width or (a.size and a.strides[1] != 4):
        raise ValueError(f"{what} must be a float32 [n_envs, {width}] array with unit column stride")
    if a.shape[0] > 1 and (a.strides[0] % 4 or a.strides[0] < 4 * width):
        raise ValueError(f"{what}: rows must be a whole number of floats apart, at least the width")
    return a.strides[0] // 4 if a.shape[0] > 1 else width


def host_scan_obs_push(state: dict, rows: np.ndarray, n_beams: int, n_mid: int, n_tail: int = 0, reset=None,
                       out: np.ndarray | None = None, **params):
    """One push on the host (f110_host_scan_obs_push) over NumPy arrays; ``state`` as
    host_scan_obs_state makes it, updated in place.  rows: float32 [N, B + M + T] and out: float32
    [N, width], either may have strided rows (unit stride inside a row); reset: uint8 / bool [N] or
    None.  Returns out."""
    B, M, T = _shape(n_beams, n_mid, n_tail)
    p = scan_obs_params(B, **params)
    width = scan_obs_width(B, M, T, **params)
    ring, head = state["ring"], state["head"]
    N = head.shape[0]
    if (ring.dtype != np.float32 or head.dtype != np.int32 or ring.shape != (N, scan_obs_depth(p), p.n_bins)
            or not ring.flags.c_contiguous or not head.flags.c_contiguous):
        raise ValueError("state must come from host_scan_obs_state with the same parameters")
    if not isinstance(rows, np.ndarray) or rows.ndim != 2 or rows.shape[0] != N:
        raise ValueError(f"rows must be a float32 [{N}, {B + M + T}] array")
    rs = _np_stride(rows, B + M + T, "rows")
    if out is None:
        out = np.empty((N, width), dtype=np.float32)
    if not isinstance(out, np.ndarray) or out.ndim != 2 or out.shape[0] != N:
        raise ValueError(f"out must be a float32 [{N}, {width}] array")
    os_ = _np_stride(out, width, "out")
    if reset is not None:
        reset = np.ascontiguousarray(np.asarray(reset).astype(np.uint8).reshape(-1))
        if reset.shape[0] != N:
            raise ValueError(f"reset must have {N} entries; got {reset.shape[0]}")
    try:
        _lib.check(_lib.load().f110_host_scan_obs_push(
            ctypes.byref(p), N, B, M, T, rows.ctypes.data, rs, None if reset is None else reset.ctypes.data,
            ring.ctypes.data, head.ctypes.data, out.ctypes.data, os_), "f110_host_scan_obs_push")
    except _lib.F110Error as exc:  # (every refusal of this entry is a bad argument)
        raise ValueError(str(exc)) from exc
    return out


def scan_obs_columns(p, mid_low=None, mid_high=None, tail_low=None, tail_high=None):
    """(low, high) float32 [width] of the compact row: [0, 1] for the pooled ranges, the given
    bounds for the kept middle and the tail columns."""
    def row(fill, mid, tail):
        rest = [np.asarray(x, np.float32) for x in (mid if p.keep_mid else None, tail) if x is not None]
        return np.concatenate([np.full(int(p.n_frames) * int(p.n_bins), fill, np.float32)] + rest)
    return row(0.0, mid_low, tail_low), row(1.0, mid_high, tail_high)


class ScanObs:
    """The compact observation of ``n_envs`` envs: the library's ring and heads on ``device`` and
    one launch per ``push`` on the current stream.  ``width`` is the compact row's width; ``low`` /
    ``high`` bound the pooled columns in [0, 1] and leave the others open (F110VectorEnv sets its
    own from the full row's bounds).  params: see scan_obs_params."""

    def __init__(self, n_envs: int, n_beams: int, n_mid: int, n_tail: int = 0, device=0, **params):
        self.handle = None
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError(f"n_envs must be at least 1; got {n_envs}")
        self.n_beams, self.n_mid, self.n_tail = _shape(n_beams, n_mid, n_tail)
        self.params = scan_obs_params(self.n_beams, **params)
        self.in_width = self.n_beams + self.n_mid + self.n_tail
        self.width = scan_obs_width(self.n_beams, self.n_mid, self.n_tail, **params)
        self.depth = scan_obs_depth(self.params)
        rest = self.width - self.params.n_frames * self.params.n_bins
        self.low, self.high = scan_obs_columns(self.params, tail_low=np.full(rest, -np.inf, np.float32),
                                               tail_high=np.full(rest, np.inf, np.float32))
        self.device = dev = cuda_device(device, "ScanObs")
        if dev.index is None:
            self.device = dev = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self.L.f110_scan_obs_create(ctypes.byref(h), dev.index, self.n_envs, self.n_beams, self.n_mid,
                                               self.n_tail, ctypes.byref(self.params)), "f110_scan_obs_create")
        self.handle = h
        self._keep = None  # a call's converted flags, alive until the stream has consumed them

    def push(self, rows: torch.Tensor, reset=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """rows: float32 [n_envs, B + M + T] on the device (unit column stride, rows may be
        strided); reset: uint8 / bool [n_envs] or None: the envs whose ring refills with this frame
        (an empty ring does anyway); out: float32 [n_envs, width] (rows may be strided; it must not
        overlap rows), a new tensor if None.  Returns out."""
        rs = f32_rows(rows, self.n_envs, self.in_width, self.device, "ScanObs.push: rows", copy_ok=False)[1]
        if out is None:
            out = torch.empty(self.n_envs, self.width, dtype=torch.float32, device=self.device)
        os_ = f32_rows(out, self.n_envs, self.width, self.device, "ScanObs.push: out", copy_ok=False)[1]
        self._keep = m = u8_rows(reset, self.n_envs, self.device, "reset")
        rc = self.L.f110_scan_obs_push(self.handle, ptr(rows), rs, ptr(m), ptr(out), os_, current_stream(self.device))
        if rc == -1:  # F110_E_INVALID
            raise ValueError(self.L.f110_last_error().decode())
        _lib.check(rc, "f110_scan_obs_push")
        return out

    def reset(self, mask=None):
        """Empty the rings of the envs with mask != 0 (None: all): their next push refills."""
        self._keep = m = u8_rows(mask, self.n_envs, self.device, "mask")
        _lib.check(self.L.f110_scan_obs_reset(self.handle, ptr(m), current_stream(self.device)), "f110_scan_obs_reset")

    def arrays(self) -> dict:
        """Device copies of the state (tests): ring [N, D, K] float32, head [N] int32."""
        from .replay import _d2d
        ring, head = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.L.f110_scan_obs_arrays(self.handle, ctypes.byref(ring), ctypes.byref(head)),
                   "f110_scan_obs_arrays")
        out = {"ring": torch.empty(self.n_envs, self.depth, self.params.n_bins, dtype=torch.float32, device=self.device),
               "head": torch.empty(self.n_envs, dtype=torch.int32, device=self.device)}
        _d2d(out["ring"], ring.value, current_stream(self.device))
        _d2d(out["head"], head.value, current_stream(self.device))
        return out

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.L.f110_scan_obs_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
