"""What every ctypes binding of the package repeats, once: pointers, the current stream, the device
argument, flag rows, float32 rows with their row stride, and the device-centerline check."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def ptr(t):
    """A tensor's or ndarray's first byte as c_void_p; None stays None."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data)


def stream(device, raw=None):
    """The current torch stream of ``device`` as c_void_p (raw: a caller's stream handle instead)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream if raw is None else raw)


def as_device(device):
    """An int (a HIP device index), a str or a torch.device as a torch.device."""
    return torch.device(device if not isinstance(device, int) else f"cuda:{device}")


def same_device(a, b):
    return a.type == b.type and (a.index or 0) == (b.index or 0)


def cuda_device(device, what):
    """as_device for an object that lives on the GPU: anything else is an F110Error."""
    dev = as_device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.F110Error(f"{what} runs on a HIP device only (no CPU path)")
    return dev


def u8_rows(t, n, device, what):
    """Flag rows (u8 or bool; anything else is converted) as a contiguous uint8 device tensor of n
    entries (n None: any number).  A contiguous bool tensor is reinterpreted and a contiguous uint8
    one taken as it is: no copy, a captured graph reads the caller's buffer.  None stays None."""
    if t is None:
        return None
    t = torch.as_tensor(t, device=device).reshape(-1)
    if t.dtype == torch.bool and t.is_contiguous():
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8 or not t.is_contiguous():
        t = t.to(torch.uint8).contiguous()
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{what} must have {n} entries; got {t.shape[0]}")
    return t


def row_stride(t):
    """The row stride, in elements, a kernel gets for the 2-D rows ``t``.  With one row torch may
    report any stride (a [1, w] tensor's can be 1), and the library refuses stride < width: the
    stride is then at least the width."""
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def f32_rows(t, n, width, device, what, copy_ok=True):
    """``t`` as float32 [n, width] rows (width None: any) of unit column stride on ``device``:
    (tensor, row stride).  copy_ok: what does not fit is converted and copied; otherwise (a kernel
    writes the rows in place) views are fine and copies are not -- a ValueError."""
    if copy_ok:
        t = torch.as_tensor(t, device=device)
        if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            t = t.to(torch.float32).reshape(t.shape[0], -1).contiguous()
    elif (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not same_device(t.device, device)
          or t.dim() != 2 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise ValueError(f"{what} must be a float32 [{n}, {width}] tensor on {device} with unit column stride "
                         "(views are fine, copies are not)")
    if t.shape[0] != n or (width is not None and t.shape[1] != width):
        raise ValueError(f"{what} must be [{n}, {'any' if width is None else width}]; got {tuple(t.shape)}")
    return t, row_stride(t)


def first_track(*candidates):
    """The first candidate that is not None (None if there is none)."""
    return next((c for c in candidates if c is not None), None)


def device_track(track, device, what, missing=None, user="the env"):
    """``track`` if it is an open device reward.CenterlineTrack on ``device`` (duck-typed: it has a
    ``device`` and a non-null ``handle``), else a ValueError: ``missing`` (default: what + " must be
    an open device reward.CenterlineTrack") or "<what> is on ..., <user> on ..."."""
    tdev = getattr(track, "device", None)
    if track is None or tdev is None or not getattr(track, "handle", None):
        raise ValueError(missing or f"{what} must be an open device reward.CenterlineTrack")
    dev = as_device(device)
    if not same_device(tdev, dev):
        raise ValueError(f"{what} is on {tdev}, {user} on {dev}")
    return track
