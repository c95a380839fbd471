"""Fused DDPG output heads (include/f110.h "learner heads", csrc/f110_ddpg.hip).

The last layer of each DDPG network and what replay() does with it
(rl_training/DDPG/agent.py):

  actor_head   fc3 -> tanh -> 0.5*(high-low)*t + 0.5*(high+low)   (:56-61)
  td_target    r + gamma * (1 - d) * critic_target.q(h)            (:302-308)
  critic_loss  td = y - critic.q(h); mean(w * td**2)               (:310-316)
  q_mean       -mean(critic.q(h))  (the actor loss)                (:321-326)

as torch.autograd.Functions over HIP kernels: one row-parallel launch
forward, a row pass and a deterministic two-pass weight reduction backward,
instead of a skinny GEMM (N = 1 or 2) and 3-10 elementwise launches.  They
run on the caller's current stream and allocate through torch, so a HIP
graph can capture them.  Device tensors only: there is no CPU path here
(DDPG on the CPU uses the plain torch modules)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _scratch(L, B, K, n, like):
    m = L.f110_ddpg_scratch_floats(B, K, n)
    if m < 0:
        raise _lib.F110Error(f"learner head: unsupported shape B={B} K={K} nout={n}")
    return torch.empty(int(m), dtype=torch.float32, device=like.device)


def _check(h, W, b):
    if not (h.is_cuda and W.is_cuda and b.is_cuda):
        raise _lib.F110Error("learner heads run on a HIP device only")
    if h.dtype != torch.float32 or W.dtype != torch.float32:
        raise _lib.F110Error("learner heads are float32")
    if h.dim() != 2 or W.dim() != 2 or h.shape[1] != W.shape[1] or b.numel() != W.shape[0]:
        raise _lib.F110Error(f"learner head shapes: h {tuple(h.shape)} W {tuple(W.shape)} b {tuple(b.shape)}")


class _ActorHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, scale, shift):
        _check(h, W, b)
        L = _lib.load()
        h, W, b = h.contiguous(), W.contiguous(), b.contiguous()
        B, K = h.shape
        n = W.shape[0]
        act = torch.empty(B, n, dtype=torch.float32, device=h.device)
        t = torch.empty_like(act)
        _lib.check(L.f110_ddpg_actor_head(_p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, n, _p(act), _p(t),
                                          _stream(h)), "f110_ddpg_actor_head")
        ctx.save_for_backward(h, W, t, scale)
        return act

    @staticmethod
    def backward(ctx, dact):
        h, W, t, scale = ctx.saved_tensors
        L = _lib.load()
        B, K = h.shape
        n = W.shape[0]
        nh, nw, nb = ctx.needs_input_grad[:3]
        dh = torch.empty_like(h) if nh else None
        dW = torch.empty_like(W) if nw else None
        db = torch.empty(n, dtype=torch.float32, device=h.device) if nb else None
        dact = dact.contiguous()
        _lib.check(L.f110_ddpg_actor_head_bwd(_p(h), _p(W), _p(t), _p(scale), _p(dact), B, K, n, _p(dh), None,
                                              _p(dW), _p(db), _p(_scratch(L, B, K, n, h)), _stream(h)),
                   "f110_ddpg_actor_head_bwd")
        return dh, dW, db, None, None


class _CriticLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, y, w):
        _check(h, W, b)
        L = _lib.load()
        h, W, b = h.contiguous(), W.contiguous(), b.contiguous()
        y, w = y.reshape(-1).contiguous(), w.reshape(-1).contiguous()
        B, K = h.shape
        td = torch.empty(B, 1, dtype=torch.float32, device=h.device)
        loss = torch.empty((), dtype=torch.float32, device=h.device)
        _lib.check(L.f110_ddpg_critic_loss(_p(h), _p(W), _p(b), _p(y), _p(w), B, K, _p(td), _p(loss),
                                           _p(_scratch(L, B, K, 1, h)), _stream(h)), "f110_ddpg_critic_loss")
        ctx.save_for_backward(h, W, td, w)
        ctx.mark_non_differentiable(td)
        return loss, td

    @staticmethod
    def backward(ctx, gloss, _gtd):
        h, W, td, w = ctx.saved_tensors
        L = _lib.load()
        B, K = h.shape
        nh, nw, nb = ctx.needs_input_grad[:3]
        dh = torch.empty_like(h) if nh else None
        dW = torch.empty_like(W) if nw else None
        db = torch.empty(1, dtype=torch.float32, device=h.device) if nb else None
        g = gloss.reshape(()).contiguous()
        _lib.check(L.f110_ddpg_critic_loss_bwd(_p(h), _p(W), _p(td), _p(w), _p(g), B, K, _p(dh), None, _p(dW),
                                               _p(db), _p(_scratch(L, B, K, 1, h)), _stream(h)), "f110_ddpg_critic_loss_bwd")
        return dh, dW, db, None, None


class _QMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, sign):
        _check(h, W, b)
        L = _lib.load()
        h, W, b = h.contiguous(), W.contiguous(), b.contiguous()
        B, K = h.shape
        loss = torch.empty((), dtype=torch.float32, device=h.device)
        _lib.check(L.f110_ddpg_q_mean(_p(h), _p(W), _p(b), float(sign), B, K, _p(loss),
                                      _p(_scratch(L, B, K, 1, h)), _stream(h)), "f110_ddpg_q_mean")
        ctx.save_for_backward(h, W)
        ctx.sign = float(sign)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        h, W = ctx.saved_tensors
        L = _lib.load()
        B, K = h.shape
        nh, nw, nb = ctx.needs_input_grad[:3]
        dh = torch.empty_like(h) if nh else None
        dW = torch.empty_like(W) if nw else None
        db = torch.empty(1, dtype=torch.float32, device=h.device) if nb else None
        g = gloss.reshape(()).contiguous()
        _lib.check(L.f110_ddpg_q_mean_bwd(_p(h), _p(W), _p(g), ctx.sign, B, K, _p(dh), None, _p(dW), _p(db),
                                          _p(_scratch(L, B, K, 1, h)), _stream(h)), "f110_ddpg_q_mean_bwd")
        return dh, dW, db, None


def actor_head(h, W, b, scale, shift):
    """0.5*(high-low) * tanh(h W^T + b) + 0.5*(high+low); scale / shift are
    those two float32 vectors."""
    return _ActorHead.apply(h, W, b, scale, shift)


def critic_loss(h, W, b, y, w):
    """(mean(w * td**2), td) with td = y - (h W^T + b); td [B, 1] is detached."""
    return _CriticLoss.apply(h, W, b, y, w)


def q_mean(h, W, b, sign: float = -1.0):
    """sign * mean(h W^T + b) (sign -1: the actor loss)."""
    return _QMean.apply(h, W, b, sign)


@torch.no_grad()
def td_target(h, W, b, r, d, gamma: float):
    """r + gamma * (1 - d) * (h W^T + b) as [B, 1] (no autograd)."""
    _check(h, W, b)
    L = _lib.load()
    h, W, b = h.contiguous(), W.contiguous(), b.contiguous()
    r, d = r.reshape(-1).contiguous(), d.reshape(-1).contiguous()
    B, K = h.shape
    y = torch.empty(B, 1, dtype=torch.float32, device=h.device)
    _lib.check(L.f110_ddpg_td_target(_p(h), _p(W), _p(b), _p(r), _p(d), float(gamma), B, K, _p(y), _stream(h)),
               "f110_ddpg_td_target")
    return y


def relu_bwd(gy, y, need_db: bool = True):
    """(threshold_backward(gy, y, 0), its column sums or None) in one pass."""
    L = _lib.load()
    gy, y = gy.contiguous(), y.contiguous()
    B, K = y.shape
    gz = torch.empty_like(y)
    db = torch.empty(K, dtype=torch.float32, device=y.device) if need_db else None
    m = L.f110_ddpg_relu_bwd_scratch_floats(B, K)
    if m < 0:
        raise _lib.F110Error(f"relu_bwd: unsupported shape B={B} K={K}")
    scratch = torch.empty(int(m), dtype=torch.float32, device=y.device) if need_db else None
    _lib.check(L.f110_ddpg_relu_bwd(_p(gy), _p(y), B, K, _p(gz), _p(db), _p(scratch), _stream(y)),
               "f110_ddpg_relu_bwd")
    return gz, db


def actor_explore_env(h, W, b, scale, shift, state_in, state_out, decay, sigma_min, low, high, seed, out, kind=0,
                      ou_x=None, theta=0.15, mu=0.0, dt=1.0, reset=None, eval_mask=None, normals_ext=None):
    """f110_ddpg_actor_explore_env (include/f110.h) on device tensors: the actor's last layer with
    per-row exploration -- Gaussian (kind 0) or OU (kind 1, ou_x float64 [B, nout] read and written)
    noise, reset / eval_mask uint8 [B] or None, normals_ext float32 [B, nout] or None -- written
    into out ([B, nout] float32, rows may be strided).  No autograd (choose_action)."""
    _check(h, W, b)
    B, K = h.shape
    n = W.shape[0]
    if out.shape != (B, n) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise _lib.F110Error("actor_explore_env: out must be [B, nout] float32 with unit column stride")
    for name, t, dt_, shape in (("ou_x", ou_x, torch.float64, (B, n)), ("reset", reset, torch.uint8, (B,)),
                                ("eval_mask", eval_mask, torch.uint8, (B,)),
                                ("normals_ext", normals_ext, torch.float32, (B, n))):
        if t is not None and (t.dtype != dt_ or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
            raise _lib.F110Error(f"actor_explore_env: {name} must be a contiguous device {dt_} tensor {shape}")
    h, W = h.contiguous(), W.contiguous()
    _lib.check(_lib.load().f110_ddpg_actor_explore_env(
        _p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, n, _p(state_in), _p(state_out),
        float(decay), float(sigma_min), _p(low), _p(high), int(seed), _p(out), out.stride(0), int(kind), _p(ou_x),
        float(theta), float(mu), float(dt), _p(reset), _p(eval_mask), _p(normals_ext), _stream(h)),
        "f110_ddpg_actor_explore_env")
    return out


def host_explore_rows(act, normals, kind, ou_x, sigma, low, high, theta=0.15, mu=0.0, dt=1.0, reset=None,
                      eval_mask=None, decay=1.0, sigma_min=0.0, call=0):
    """f110_host_explore_rows over NumPy arrays: the per-row epilogue of f110_ddpg_actor_explore_env
    on the CPU, on given actions act [n, nout] float32 and draws normals [n, nout] float32; ou_x
    (float64 [n, nout], kind 1) is updated in place.  Returns (out [n, nout] float32, the decayed
    (sigma, call index) pair)."""
    act = np.ascontiguousarray(act, np.float32)
    n, nout = act.shape
    normals = np.ascontiguousarray(normals, np.float32)
    low, high = np.ascontiguousarray(low, np.float32), np.ascontiguousarray(high, np.float32)
    if normals.shape != act.shape or low.shape != (nout,) or high.shape != (nout,):
        raise ValueError("host_explore_rows: normals must match act, low / high must have nout entries")
    if ou_x is not None and (ou_x.dtype != np.float64 or ou_x.shape != act.shape or not ou_x.flags.c_contiguous):
        raise ValueError("host_explore_rows: ou_x must be a C-contiguous float64 array shaped like act")
    masks = []
    for m in (reset, eval_mask):
        m = None if m is None else np.ascontiguousarray(m, np.uint8)
        if m is not None and m.shape != (n,):
            raise ValueError("host_explore_rows: reset / eval_mask must have one entry per row")
        masks.append(m)
    st_in, st_out = np.array([sigma, float(call)], np.float64), np.zeros(2, np.float64)
    out = np.empty_like(act)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(_lib.load().f110_host_explore_rows(P(act), P(normals), n, nout, int(kind), P(ou_x), float(theta),
                                                  float(mu), float(dt), P(masks[0]), P(masks[1]), P(st_in), P(st_out),
                                                  float(decay), float(sigma_min), P(low), P(high), P(out)),
               "f110_host_explore_rows")
    return out, (float(st_out[0]), float(st_out[1]))


def td3_target_action(h, W, b, scale, shift, policy_noise, noise_clip, low, high, seed=0, counter=None,
                      normals_ext=None):
    """f110_td3_target_action (include/f110.h) on device tensors: the target actor's last layer with
    target-policy smoothing, [B, nout] float32.  The draws are normals_ext ([B, nout] float32) when
    given, else the device stream of (seed, counter[0]); counter is a device int64 tensor that is
    only read.  No autograd."""
    _check(h, W, b)
    B, K = h.shape
    n = W.shape[0]
    if normals_ext is not None and (normals_ext.dtype != torch.float32 or tuple(normals_ext.shape) != (B, n)
                                    or not normals_ext.is_contiguous() or not normals_ext.is_cuda):
        raise _lib.F110Error(f"td3_target_action: normals_ext must be a contiguous device float32 tensor {(B, n)}")
    if counter is not None and (counter.dtype != torch.int64 or not counter.is_cuda):
        raise _lib.F110Error("td3_target_action: counter must be a device int64 tensor")
    h, W = h.contiguous(), W.contiguous()
    out = torch.empty(B, n, dtype=torch.float32, device=h.device)
    _lib.check(_lib.load().f110_td3_target_action(
        _p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, n, float(policy_noise), float(noise_clip), _p(low),
        _p(high), int(seed) & ((1 << 64) - 1), _p(counter), _p(normals_ext), _p(out), _stream(h)),
        "f110_td3_target_action")
    return out


def td3_critic_step(ht1, Wt1, bt1, ht2, Wt2, bt2, r, d, gamma, h1, W1, b1, h2, W2, b2, w, g, dh_masks=(None, None),
                    want_dh=True):
    """f110_td3_critic_step (include/f110.h) on device tensors.  Returns a dict: td (the PER
    priority, [B, 1]), dq1 / dq2 [B, 1], dh1 / dh2 [B, K] (want_dh; masked by dh_masks) and part
    (the loss is part.sum() / B).  No autograd."""
    for hh, WW, bb in ((ht1, Wt1, bt1), (ht2, Wt2, bt2), (h1, W1, b1), (h2, W2, b2)):
        _check(hh, WW, bb)
    L = _lib.load()
    B, K = h1.shape
    dev = h1.device
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"td": e(B, 1), "dq1": e(B, 1), "dq2": e(B, 1), "dh1": e(B, K) if want_dh else None,
           "dh2": e(B, K) if want_dh else None, "part": e(L.f110_ddpg_row_blocks(B))}
    r, d, w = r.reshape(-1).contiguous(), d.reshape(-1).contiguous(), w.reshape(-1).contiguous()
    _lib.check(L.f110_td3_critic_step(_p(ht1), _p(Wt1), _p(bt1), _p(ht2), _p(Wt2), _p(bt2), _p(r), _p(d),
                                      float(gamma), _p(h1), _p(W1), _p(b1), _p(h2), _p(W2), _p(b2), _p(w), _p(g), B,
                                      K, _p(out["td"]), _p(out["dh1"]), _p(dh_masks[0]), _p(out["dh2"]),
                                      _p(dh_masks[1]), _p(out["dq1"]), _p(out["dq2"]), _p(out["part"]), _stream(h1)),
               "f110_td3_critic_step")
    return out


def host_td3_smooth_rows(act, normals, policy_noise, noise_clip, scale, low, high):
    """f110_host_td3_smooth_rows over NumPy arrays: f110_td3_target_action's per-row epilogue on the
    CPU, on given actions act [n, nout] float32 and draws normals [n, nout] float32."""
    act = np.ascontiguousarray(act, np.float32)
    n, nout = act.shape
    normals = np.ascontiguousarray(normals, np.float32)
    scale, low, high = (np.ascontiguousarray(v, np.float32) for v in (scale, low, high))
    if normals.shape != act.shape or any(v.shape != (nout,) for v in (scale, low, high)):
        raise ValueError("host_td3_smooth_rows: normals must match act; scale / low / high must have nout entries")
    out = np.empty_like(act)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(_lib.load().f110_host_td3_smooth_rows(P(act), P(normals), n, nout, float(policy_noise),
                                                     float(noise_clip), P(scale), P(low), P(high), P(out)),
               "f110_host_td3_smooth_rows")
    return out


def host_td3_rows(r, d, gamma, q1t, q2t, q1, q2, w, g=1.0):
    """f110_host_td3_rows over NumPy arrays ([B] float32 each): f110_td3_critic_step's row rule on
    the CPU.  Returns a dict of td1, td2, dq1, dq2, prio, wl ([B] float32)."""
    a = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (r, d, q1t, q2t, q1, q2, w)]
    B = a[0].shape[0]
    if any(v.shape != (B,) for v in a):
        raise ValueError("host_td3_rows: every input must have B entries")
    out = {k: np.empty(B, np.float32) for k in ("td1", "td2", "dq1", "dq2", "prio", "wl")}
    P = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    _lib.check(_lib.load().f110_host_td3_rows(P(a[0]), P(a[1]), float(gamma), P(a[2]), P(a[3]), P(a[4]), P(a[5]),
                                              P(a[6]), float(g), B, *(P(out[k]) for k in out)),
               "f110_host_td3_rows")
    return out
