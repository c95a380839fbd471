"""Prioritized experience replay in device memory.

Mirrors rl_training/DDPG/replay_buffer.py:PrioritizedExperienceReplayBuffer
(:6-135) -- same constructor arguments and defaults, ``add`` / ``sample`` /
``update_priorities`` / ``len`` -- for batches of transitions held as device
tensors.  Every call is libf110's ``f110_replay_*`` on the current torch
stream; nothing goes through the host on the per-step path.

    rb = DeviceReplayBuffer(buffer_size=1 << 20, batch_size=4096, obs_dim=1088, act_dim=2, device=0)
    rb.add(obs, act, rew, next_obs, done, mask=~reset)    # [n, 1088], [n, 2], [n], [n, 1088], [n]
    idx, batch, w = rb.sample(beta=0.4)                    # batch: states, actions, rewards, next_states, dones
    rb.update_priorities(idx, td, td_errors=True, add_eps=1e-5)   # |td| + eps (agent.py:337)

Sampling without replacement has the distribution of numpy's
``Generator.choice(replace=False, p=...)`` (an ordered successive sample);
the draws themselves come from a device Philox stream, not PCG64.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())



def _as_u8(t: torch.Tensor) -> torch.Tensor:
    """Flat uint8 flags; a contiguous bool tensor is reinterpreted (no copy)."""
    t = t.reshape(-1)
    if t.dtype == torch.bool and t.is_contiguous():
        return t.view(torch.uint8)
    return t.to(torch.uint8).contiguous()

class DeviceReplayBuffer:
    def __init__(self, buffer_size: int, batch_size: int, alpha: float = 0.6, seed: int = 42,
                 priority_epsilon: float = 1e-6, obs_dim: int = 1088, act_dim: int = 2, device=0,
                 max_add: int | None = None):
        if batch_size <= 0 or buffer_size <= 0:
            raise ValueError("buffer_size and batch_size must be positive")  # replay_buffer.py:26
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.F110Error("DeviceReplayBuffer runs on a HIP device only (no CPU path)")
        self.device = dev
        self.L = _lib.load()
        self._buffer_size = int(buffer_size)
        self._batch_size = int(batch_size)
        self._alpha = float(alpha)
        self._eps = float(priority_epsilon)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.max_add = int(max_add or min(self._buffer_size, 1 << 16))
        h = ctypes.c_void_p()
        _lib.check(self.L.f110_replay_create(ctypes.byref(h), dev.index or 0, self._buffer_size, self.obs_dim,
                                             self.act_dim, self._batch_size, self.max_add, self._alpha, self._eps,
                                             int(seed) & 0xFFFFFFFFFFFFFFFF), "f110_replay_create")
        self.handle = h
        kw = dict(device=dev)
        B = self._batch_size
        self.idx = torch.empty(B, dtype=torch.int64, **kw)
        self.weights = torch.empty(B, dtype=torch.float32, **kw)
        self.batch = {
            "states": torch.empty(B, self.obs_dim, dtype=torch.float32, **kw),
            "actions": torch.empty(B, self.act_dim, dtype=torch.float32, **kw),
            "rewards": torch.empty(B, dtype=torch.float32, **kw),
            "next_states": torch.empty(B, self.obs_dim, dtype=torch.float32, **kw),
            "dones": torch.empty(B, dtype=torch.float32, **kw),
        }
        self._added = 0  # host upper bound of len() (masked rows may not be stored)
        self._keep = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------
    def __len__(self) -> int:
        """replay_buffer.py:42-43 (waits for the stream)."""
        n = ctypes.c_int64()
        _lib.check(self.L.f110_replay_length(self.handle, ctypes.byref(n), None, self._stream()),
                   "f110_replay_length")
        return int(n.value)

    def add(self, states, actions, rewards, next_states, dones=None, mask=None, priority=None):
        """n add() calls (replay_buffer.py:48-71) in row order, priority = the
        current max (1.0 when empty) or ``priority`` [n].  Rows with mask == 0
        are not stored."""
        s = self._rows(states, self.obs_dim)
        ns = self._rows(next_states, self.obs_dim)
        a = self._rows(actions, self.act_dim)
        n = s.shape[0]
        r = torch.as_tensor(rewards, device=self.device).reshape(-1).to(torch.float32).contiguous()
        d = None if dones is None else _as_u8(torch.as_tensor(dones, device=self.device))
        m = None if mask is None else _as_u8(torch.as_tensor(mask, device=self.device))
        pr = None if priority is None else \
            torch.as_tensor(priority, device=self.device).reshape(-1).to(torch.float32).contiguous()
        if (pr is not None and pr.shape[0] != n) or ns.shape[0] != n or a.shape[0] != n or r.shape[0] != n or (d is not None and d.shape[0] != n) or \
                (m is not None and m.shape[0] != n):
            raise ValueError("add: every input needs the same number of rows")
        self._keep = (s, ns, a, r, d, m, pr)  # alive until the stream has consumed them
        for lo in range(0, n, self.max_add):
            hi = min(n, lo + self.max_add)
            _lib.check(self.L.f110_replay_add(
                self.handle, _p(s[lo:hi]), s.stride(0), _p(a[lo:hi]), a.stride(0), _p(r[lo:hi]), _p(ns[lo:hi]),
                ns.stride(0), _p(None if d is None else d[lo:hi]), _p(None if pr is None else pr[lo:hi]),
                _p(None if m is None else m[lo:hi]), hi - lo,
                self._stream()), "f110_replay_add")
        self._added += n

    def note_added(self, n: int):
        """A captured add / add_env of n rows was replayed (or rows reached the ring some other way
        than through these methods): the host's bound on len() follows."""
        self._added += int(n)

    def add_env(self, states, actions, rewards, next_states, terminated, was_reset):
        """add() of a vector env's raw step outputs (f110_replay_add_env): rewards
        float64, terminated / was_reset uint8 device tensors as the simulator
        writes them; rows with was_reset != 0 are not stored.  No dtype
        conversions on the torch side."""
        s = self._rows(states, self.obs_dim)
        ns = self._rows(next_states, self.obs_dim)
        a = self._rows(actions, self.act_dim)
        n = s.shape[0]
        r, d, m = rewards.reshape(-1), terminated.reshape(-1), was_reset.reshape(-1)
        if r.dtype != torch.float64 or d.dtype != torch.uint8 or m.dtype != torch.uint8:
            raise TypeError("add_env: rewards float64, terminated and was_reset uint8")
        if not (r.is_contiguous() and d.is_contiguous() and m.is_contiguous()):
            raise ValueError("add_env: contiguous rewards / flags")
        if ns.shape[0] != n or a.shape[0] != n or r.shape[0] != n or d.shape[0] != n or m.shape[0] != n:
            raise ValueError("add_env: every input needs the same number of rows")
        self._keep = (s, ns, a, r, d, m)  # alive until the stream has consumed them
        for lo in range(0, n, self.max_add):
            hi = min(n, lo + self.max_add)
            _lib.check(self.L.f110_replay_add_env(
                self.handle, _p(s[lo:hi]), s.stride(0), _p(a[lo:hi]), a.stride(0), _p(r[lo:hi]), _p(ns[lo:hi]),
                ns.stride(0), _p(d[lo:hi]), _p(m[lo:hi]), hi - lo, self._stream()), "f110_replay_add_env")
        self._added += n

    def _rows(self, x, width):
        t = torch.as_tensor(x, device=self.device)
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        t = t.reshape(-1, width)
        if t.stride(1) != 1:
            t = t.contiguous()
        return t

    def sample(self, beta: float = 0.4, batch_size: int | None = None, gather: bool = True):
        """replay_buffer.py:76-116: (idxs [B] int64, batch dict or None, weights [B] float32), device
        tensors.  The returned tensors are reused by the next sample()."""
        if self._added == 0:
            raise ValueError("Cannot sample from an empty buffer.")  # :83-84
        B = int(batch_size or self._batch_size)
        if B > self._batch_size:
            raise ValueError("batch_size above the buffer's batch_size")
        b = self.batch
        _lib.check(self.L.f110_replay_sample(
            self.handle, B, float(beta), _p(self.idx), _p(self.weights),
            *((_p(b["states"]), _p(b["actions"]), _p(b["rewards"]), _p(b["next_states"]), _p(b["dones"]))
              if gather else (None,) * 5), self._stream()), "f110_replay_sample")
        if B == self._batch_size:
            return self.idx, (b if gather else None), self.weights
        return self.idx[:B], ({k: v[:B] for k, v in b.items()} if gather else None), self.weights[:B]

    def update_priorities(self, idxs, priorities, td_errors: bool = False, add_eps: float = 0.0):
        """update_priorities(idxs, priorities) (replay_buffer.py:121-135).
        td_errors=True takes TD errors and stores agent.replay's
        |td| + add_eps (agent.py:337) without a separate kernel."""
        i = torch.as_tensor(idxs, device=self.device).reshape(-1).to(torch.int64).contiguous()
        t = torch.as_tensor(priorities, device=self.device).reshape(-1).to(torch.float32).contiguous()
        if i.shape != t.shape:
            raise ValueError("update_priorities: idxs and priorities differ in length")
        self._keep_u = (i, t)
        _lib.check(self.L.f110_replay_update_priorities(self.handle, _p(i), _p(t), i.shape[0], int(bool(td_errors)),
                                                        float(add_eps), self._stream()),
                   "f110_replay_update_priorities")

    # ------------------------------------------------------------------
    def arrays(self, names=("priority", "states", "actions", "rewards", "next_states", "dones")):
        """Device copies of the stored arrays: priority [cap], states / next_states [cap, D],
        actions [cap, A], rewards / dones [cap] (checkpoints, tests)."""
        ptrs = [ctypes.c_void_p() for _ in range(6)]
        _lib.check(self.L.f110_replay_arrays(self.handle, *[ctypes.byref(p) for p in ptrs]), "f110_replay_arrays")
        cap, D, A = self._buffer_size, self.obs_dim, self.act_dim
        shapes = {"priority": (cap,), "states": (cap, D), "actions": (cap, A), "rewards": (cap,),
                  "next_states": (cap, D), "dones": (cap,)}
        order = ["priority", "states", "actions", "rewards", "next_states", "dones"]
        out = {}
        for n in names:
            t = torch.empty(shapes[n], dtype=torch.float32, device=self.device)
            _d2d(t, ptrs[order.index(n)].value, self._stream())
            out[n] = t
        return out

    def priorities(self) -> torch.Tensor:
        return self.arrays(("priority",))["priority"]

    # ---- the select, for tests (f110_replay_select_keys / f110_replay_select_state) ----
    def select_keys(self, keys, beta: float = 0.4, batch_size: int | None = None):
        """sample()'s selection over ``keys`` [len] (uint32 patterns, one per stored row) in place
        of the drawn ones: (idxs [B] int64 ascending, weights [B] float32), no gather."""
        k = torch.as_tensor(keys, device=self.device).reshape(-1)
        if k.dtype != torch.uint32:
            k = k.to(torch.int64).to(torch.uint32)
        k = k.contiguous()
        B = int(batch_size or self._batch_size)
        self._keep_k = k
        _lib.check(self.L.f110_replay_select_keys(self.handle, _p(k), k.shape[0], B, float(beta), _p(self.idx),
                                                  _p(self.weights), self._stream()), "f110_replay_select_keys")
        return self.idx[:B], self.weights[:B]

    def _select_state(self, **out):
        _lib.check(self.L.f110_replay_select_state(
            self.handle, *[None if out.get(n) is None else ctypes.byref(out[n])
                           for n in ("keys", "wt", "prefix", "kleft", "n_lt", "den", "overflow")], self._stream()),
            "f110_replay_select_state")

    def keys(self) -> torch.Tensor:
        """[cap] uint32 copy of the last sample's keys (rows past len() hold no key)."""
        p = ctypes.c_void_p()
        self._select_state(keys=p)
        t = torch.empty(self._buffer_size, dtype=torch.uint32, device=self.device)
        _d2d(t, p.value, self._stream())
        return t

    def sampling_weights(self) -> torch.Tensor:
        """[cap] float64 copy of (priority + eps)^alpha, as the sampler caches it."""
        p = ctypes.c_void_p()
        self._select_state(wt=p)
        t = torch.empty(self._buffer_size, dtype=torch.float64, device=self.device)
        _d2d(t, p.value, self._stream())
        return t

    def select_state(self) -> dict:
        """The last without-replacement sample's threshold key (prefix), rows still to take among
        its ties (kleft), rows below it (n_lt), sum of the sampling weights (den), and the
        tie-list overflows so far (waits for the stream)."""
        u = {n: ctypes.c_uint32() for n in ("prefix", "kleft", "n_lt", "overflow")}
        den = ctypes.c_double()
        self._select_state(den=den, **u)
        return {"prefix": u["prefix"].value, "kleft": u["kleft"].value, "n_lt": u["n_lt"].value,
                "den": den.value, "overflow": u["overflow"].value}

    def tie_overflows(self) -> int:
        """Samples so far that met more keys equal to the threshold than the tie list holds."""
        return self.select_state()["overflow"]

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.L.f110_replay_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NStepAccumulator:
    """N-step returns in front of a DeviceReplayBuffer (include/f110.h, "n-step returns"): per env a
    device window of at most ``n_step`` pending (s, a, running return) entries.  ``push`` takes a
    vector env's raw step outputs as ``add_env`` does and appends what leaves the windows to the
    ring: an entry with its n rewards, or every entry of an env whose episode ends.  A stored row's
    done column is the effective done 1 - gamma^(k-1) (1 - done), so the one-step learner
    bootstraps it with gamma^k.  All on the current torch stream; nothing goes through the host."""

    def __init__(self, n_envs: int, n_step: int, gamma: float, obs_dim: int = 1088, act_dim: int = 2, device=0):
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.L = _lib.load()
        self.n_envs, self.n_step, self.gamma = int(n_envs), int(n_step), float(gamma)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.handle = None
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.F110Error("NStepAccumulator runs on a HIP device only (no CPU path)")
        self.device = dev
        h = ctypes.c_void_p()
        _lib.check(self.L.f110_nstep_create(ctypes.byref(h), dev.index or 0, self.n_envs, self.n_step, self.gamma,
                                            self.obs_dim, self.act_dim), "f110_nstep_create")
        self.handle = h
        self._keep = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def push(self, memory: DeviceReplayBuffer, states, actions, rewards, next_states, terminated, truncated,
             was_reset):
        """One vector step into the windows; the emitted rows into ``memory``.  rewards float64,
        terminated / truncated / was_reset uint8 device tensors as the simulator writes them
        (truncated may be None: no episode limits); ``n_envs`` rows each."""
        s = memory._rows(states, self.obs_dim)
        ns = memory._rows(next_states, self.obs_dim)
        a = memory._rows(actions, self.act_dim)
        r, d, m = rewards.reshape(-1), terminated.reshape(-1), was_reset.reshape(-1)
        t = None if truncated is None else truncated.reshape(-1)
        if r.dtype != torch.float64 or d.dtype != torch.uint8 or m.dtype != torch.uint8 or \
                (t is not None and t.dtype != torch.uint8):
            raise TypeError("push: rewards float64, terminated, truncated and was_reset uint8")
        if not (r.is_contiguous() and d.is_contiguous() and m.is_contiguous() and (t is None or t.is_contiguous())):
            raise ValueError("push: contiguous rewards / flags")
        n = self.n_envs
        if any(x.shape[0] != n for x in (s, ns, a, r, d, m)) or (t is not None and t.shape[0] != n):
            raise ValueError(f"push: every input needs n_envs = {n} rows")
        self._keep = (s, ns, a, r, d, t, m)  # alive until the stream has consumed them
        _lib.check(self.L.f110_nstep_push(self.handle, memory.handle, _p(s), s.stride(0), _p(a), a.stride(0), _p(r),
                                          _p(ns), ns.stride(0), _p(d), _p(t), _p(m), self._stream()),
                   "f110_nstep_push")
        memory.note_added(n)  # an upper bound: emitted rows never outnumber pushed rows in total

    def reset(self, env_mask=None):
        """Drop the windows of the envs with env_mask != 0 (None: all); nothing is emitted."""
        m = None if env_mask is None else _as_u8(torch.as_tensor(env_mask, device=self.device))
        if m is not None and m.shape[0] != self.n_envs:
            raise ValueError("reset: env_mask needs n_envs entries")
        self._keep_m = m
        _lib.check(self.L.f110_nstep_reset(self.handle, _p(m), self._stream()), "f110_nstep_reset")

    def arrays(self):
        """Device copies of the windows (tests): len, head [N] int32, ret [N, n] float64, k [N, n]
        int32, obs [N, n, D], act [N, n, A]; entry i of env e sits in slot (head + i) % n."""
        ptrs = [ctypes.c_void_p() for _ in range(6)]
        _lib.check(self.L.f110_nstep_arrays(self.handle, *[ctypes.byref(p) for p in ptrs]), "f110_nstep_arrays")
        N, n = self.n_envs, self.n_step
        spec = [("len", (N,), torch.int32), ("head", (N,), torch.int32), ("ret", (N, n), torch.float64),
                ("k", (N, n), torch.int32), ("obs", (N, n, self.obs_dim), torch.float32),
                ("act", (N, n, self.act_dim), torch.float32)]
        out = {}
        for (name, shape, dt), p in zip(spec, ptrs):
            t = torch.empty(shape, dtype=dt, device=self.device)
            _d2d(t, p.value, self._stream())
            out[name] = t
        return out

    def pending(self) -> torch.Tensor:
        """[n_envs] int32 copy of the window lengths."""
        p = ctypes.c_void_p()
        _lib.check(self.L.f110_nstep_arrays(self.handle, ctypes.byref(p), None, None, None, None, None),
                   "f110_nstep_arrays")
        t = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        _d2d(t, p.value, self._stream())
        return t

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.L.f110_nstep_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ActionRepeat:
    """Action repeat around a vector env's step (include/f110.h, "action repeat"): per env a device
    phase, the block's first observation and action, and a running return.  ``hold`` runs before the
    env step: envs whose decision is due keep the policy's action and latch it with the observation;
    the others get their held action written over the policy's.  ``push`` runs after it and appends
    one row per finished block to the ring -- a block is finished after ``repeat`` steps or when its
    episode ends -- with the effective done 1 - gamma^(k-1) (1 - done), so the one-step learner
    bootstraps it with gamma^k.  All on the current torch stream; nothing goes through the host."""

    def __init__(self, n_envs: int, repeat: int, gamma: float, obs_dim: int = 1088, act_dim: int = 2, device=0):
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.L = _lib.load()
        self.n_envs, self.repeat, self.gamma = int(n_envs), int(repeat), float(gamma)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.handle = None
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.F110Error("ActionRepeat runs on a HIP device only (no CPU path)")
        self.device = dev
        h = ctypes.c_void_p()
        _lib.check(self.L.f110_repeat_create(ctypes.byref(h), dev.index or 0, self.n_envs, self.repeat, self.gamma,
                                             self.obs_dim, self.act_dim), "f110_repeat_create")
        self.handle = h
        self.decision = torch.zeros(self.n_envs, dtype=torch.uint8, device=dev)  # written by the last hold
        self._keep = self._keep_h = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, x, width, what):
        """x as [n_envs, width] float32 rows of unit inner stride, WITHOUT a copy (hold writes in place)."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device.type != "cuda" or \
                (x.device.index or 0) != (self.device.index or 0):
            raise TypeError(f"{what}: a float32 tensor on {self.device}")
        if x.dim() != 2 or x.shape[1] != width or x.stride(1) != 1 or x.stride(0) < width:
            raise ValueError(f"{what}: [n_envs, {width}] rows of unit inner stride (views are fine, copies are not)")
        if x.shape[0] != self.n_envs:
            raise ValueError(f"{what}: every input needs n_envs = {self.n_envs} rows")
        return x

    def hold(self, obs, act):
        """Before the env step.  obs [n_envs, obs_dim], act [n_envs, act_dim]: float32 device
        tensors or strided row views of them; act is rewritten in place and returned.
        ``decision`` [n_envs] uint8 is 1 where the policy's action was kept."""
        s = self._rows(obs, self.obs_dim, "hold: obs")
        a = self._rows(act, self.act_dim, "hold: act")
        self._keep_h = (s, a)  # alive until the stream has consumed them
        _lib.check(self.L.f110_repeat_hold(self.handle, _p(s), s.stride(0), _p(a), a.stride(0), _p(self.decision),
                                           self._stream()), "f110_repeat_hold")
        return act

    def push(self, memory: DeviceReplayBuffer, rewards, next_obs, terminated, truncated, was_reset):
        """After the env step: one vector step into the blocks; the finished blocks into ``memory``.
        rewards float64, terminated / truncated / was_reset uint8 device tensors as the simulator
        writes them (truncated may be None: no episode limits); ``n_envs`` rows each."""
        ns = memory._rows(next_obs, self.obs_dim)
        r, d, m = rewards.reshape(-1), terminated.reshape(-1), was_reset.reshape(-1)
        t = None if truncated is None else truncated.reshape(-1)
        if r.dtype != torch.float64 or d.dtype != torch.uint8 or m.dtype != torch.uint8 or \
                (t is not None and t.dtype != torch.uint8):
            raise TypeError("push: rewards float64, terminated, truncated and was_reset uint8")
        if not (r.is_contiguous() and d.is_contiguous() and m.is_contiguous() and (t is None or t.is_contiguous())):
            raise ValueError("push: contiguous rewards / flags")
        n = self.n_envs
        if any(x.shape[0] != n for x in (ns, r, d, m)) or (t is not None and t.shape[0] != n):
            raise ValueError(f"push: every input needs n_envs = {n} rows")
        self._keep = (ns, r, d, t, m)  # alive until the stream has consumed them
        _lib.check(self.L.f110_repeat_push(self.handle, memory.handle, _p(r), _p(ns), ns.stride(0), _p(d), _p(t), _p(m),
                                           self._stream()), "f110_repeat_push")
        memory.note_added(n)  # an upper bound: at most one row per env and push

    def reset(self, env_mask=None):
        """A decision is due at the next hold for the envs with env_mask != 0 (None: all); their
        running blocks are dropped and nothing is emitted."""
        m = None if env_mask is None else _as_u8(torch.as_tensor(env_mask, device=self.device))
        if m is not None and m.shape[0] != self.n_envs:
            raise ValueError("reset: env_mask needs n_envs entries")
        self._keep_m = m
        _lib.check(self.L.f110_repeat_reset(self.handle, _p(m), self._stream()), "f110_repeat_reset")

    def arrays(self):
        """Device copies of the state (tests): k [N] int32, ret [N] float64, obs [N, D], act [N, A]."""
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        _lib.check(self.L.f110_repeat_arrays(self.handle, *[ctypes.byref(p) for p in ptrs]), "f110_repeat_arrays")
        N = self.n_envs
        spec = [("k", (N,), torch.int32), ("ret", (N,), torch.float64), ("obs", (N, self.obs_dim), torch.float32),
                ("act", (N, self.act_dim), torch.float32)]
        out = {}
        for (name, shape, dt), p in zip(spec, ptrs):
            t = torch.empty(shape, dtype=dt, device=self.device)
            _d2d(t, p.value, self._stream())
            out[name] = t
        return out

    def phase(self) -> torch.Tensor:
        """[n_envs] int32 copy of the phases (0: a decision is due)."""
        p = ctypes.c_void_p()
        _lib.check(self.L.f110_repeat_arrays(self.handle, ctypes.byref(p), None, None, None), "f110_repeat_arrays")
        t = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        _d2d(t, p.value, self._stream())
        return t

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.L.f110_repeat_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_repeat_state(n_envs: int, obs_dim: int, act_dim: int) -> dict:
    """Fresh host action-repeat state in f110_repeat_arrays' layout."""
    import numpy as np
    N = int(n_envs)
    return {"k": np.zeros(N, np.int32), "ret": np.zeros(N, np.float64), "obs": np.zeros((N, obs_dim), np.float32),
            "act": np.zeros((N, act_dim), np.float32)}


def host_repeat_hold(state: dict, obs, act):
    """One hold on the host (f110_host_repeat_hold) over NumPy arrays; ``state`` as
    ``host_repeat_state`` makes it, updated in place.  Returns (act, decision): the action rows the
    env is to step with (a new array) and the uint8 decision mask."""
    import numpy as np
    L = _lib.load()
    N, D = state["obs"].shape
    A = state["act"].shape[1]
    obs = np.ascontiguousarray(obs, np.float32).reshape(N, D)
    act = np.array(act, np.float32, order="C").reshape(N, A)  # (a copy: the caller's rows stay)
    decision = np.empty(N, np.uint8)
    _lib.check(L.f110_host_repeat_hold(N, D, A, *[ctypes.c_void_p(x.ctypes.data) for x in
                                                  (state["k"], state["obs"], state["act"], obs, act, decision)]),
               "f110_host_repeat_hold")
    return act, decision


def host_repeat_push(state: dict, repeat, gamma, reward, next_obs, terminated, truncated, was_reset,
                     capacity: int = 0):
    """One push on the host (f110_host_repeat_push) over NumPy arrays.  Returns the emitted rows
    (obs, act, reward, next_obs, done) in the order the device appends them."""
    import numpy as np
    L = _lib.load()
    N, D = state["obs"].shape
    A = state["act"].shape[1]
    next_obs = np.ascontiguousarray(next_obs, np.float32).reshape(N, D)
    reward = np.ascontiguousarray(reward, np.float64).reshape(N)
    flags = [None if f is None else np.ascontiguousarray(f, np.uint8).reshape(N)
             for f in (terminated, truncated, was_reset)]
    out = [np.empty((N, D), np.float32), np.empty((N, A), np.float32), np.empty(N, np.float32),
           np.empty((N, D), np.float32), np.empty(N, np.float32)]
    cnt = ctypes.c_int64()

    def ptr(x):
        return None if x is None else ctypes.c_void_p(x.ctypes.data)
    _lib.check(L.f110_host_repeat_push(N, int(repeat), float(gamma), D, A, int(capacity),
                                       *[ptr(state[q]) for q in ("k", "ret", "obs", "act")], ptr(reward),
                                       ptr(next_obs), *[ptr(f) for f in flags], *[ptr(x) for x in out],
                                       ctypes.byref(cnt)), "f110_host_repeat_push")
    return tuple(x[:cnt.value] for x in out)


def host_nstep(state: dict, gamma, obs, act, reward, next_obs, terminated, truncated, was_reset, capacity: int = 0):
    """One push on the host (f110_host_nstep) over NumPy arrays.  ``state``: the windows, as
    ``host_nstep_state`` makes them, updated in place.  Returns the emitted rows
    (obs, act, reward, next_obs, done) in the order the device appends them."""
    import numpy as np
    L = _lib.load()
    N, n = state["ret"].shape
    D, A = state["obs"].shape[2], state["act"].shape[2]
    obs, next_obs = (np.ascontiguousarray(x, np.float32).reshape(N, D) for x in (obs, next_obs))
    act = np.ascontiguousarray(act, np.float32).reshape(N, A)
    reward = np.ascontiguousarray(reward, np.float64).reshape(N)
    flags = [None if f is None else np.ascontiguousarray(f, np.uint8).reshape(N)
             for f in (terminated, truncated, was_reset)]
    out = [np.empty((N * n, D), np.float32), np.empty((N * n, A), np.float32), np.empty(N * n, np.float32),
           np.empty((N * n, D), np.float32), np.empty(N * n, np.float32)]
    cnt = ctypes.c_int64()

    def ptr(x):
        return None if x is None else ctypes.c_void_p(x.ctypes.data)
    _lib.check(L.f110_host_nstep(N, n, float(gamma), D, A, int(capacity),
                                 *[ptr(state[q]) for q in ("len", "head", "ret", "k", "obs", "act")],
                                 ptr(obs), ptr(act), ptr(reward), ptr(next_obs), *[ptr(f) for f in flags],
                                 *[ptr(x) for x in out], ctypes.byref(cnt)), "f110_host_nstep")
    return tuple(x[:cnt.value] for x in out)


def host_nstep_state(n_envs: int, n_step: int, obs_dim: int, act_dim: int) -> dict:
    """Fresh host windows in f110_nstep_arrays' layout."""
    import numpy as np
    N, n = int(n_envs), int(n_step)
    return {"len": np.zeros(N, np.int32), "head": np.zeros(N, np.int32), "ret": np.zeros((N, n), np.float64),
            "k": np.zeros((N, n), np.int32), "obs": np.zeros((N, n, obs_dim), np.float32),
            "act": np.zeros((N, n, act_dim), np.float32)}


_hip = None


def _d2d(dst: torch.Tensor, src_ptr: int, stream) -> None:
    """hipMemcpyAsync device-to-device from library-owned memory into a tensor."""
    global _hip
    if _hip is None:
        _lib.load()
        _hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libf110 and torch already share (by SONAME)
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                        ctypes.c_void_p]
        _hip.hipMemcpyAsync.restype = ctypes.c_int
    rc = _hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src_ptr),
                             dst.numel() * dst.element_size(), 3, stream)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise _lib.F110Error(f"hipMemcpyAsync failed ({rc})")
