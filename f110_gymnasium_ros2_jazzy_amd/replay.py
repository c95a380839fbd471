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
from ._dev import cuda_device, f32_rows, ptr, same_device, stream, u8_rows


class DeviceReplayBuffer:
    def __init__(self, buffer_size: int, batch_size: int, alpha: float = 0.6, seed: int = 42,
                 priority_epsilon: float = 1e-6, obs_dim: int = 1088, act_dim: int = 2, device=0,
                 max_add: int | None = None):
        if batch_size <= 0 or buffer_size <= 0:
            raise ValueError("buffer_size and batch_size must be positive")  # replay_buffer.py:26
        self.device = dev = cuda_device(device, "DeviceReplayBuffer")
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
        return stream(self.device)

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
        d = u8_rows(dones, None, self.device, "dones")
        m = u8_rows(mask, None, self.device, "mask")
        pr = None if priority is None else \
            torch.as_tensor(priority, device=self.device).reshape(-1).to(torch.float32).contiguous()
        if (pr is not None and pr.shape[0] != n) or ns.shape[0] != n or a.shape[0] != n or r.shape[0] != n or (d is not None and d.shape[0] != n) or \
                (m is not None and m.shape[0] != n):
            raise ValueError("add: every input needs the same number of rows")
        self._keep = (s, ns, a, r, d, m, pr)  # alive until the stream has consumed them
        for lo in range(0, n, self.max_add):
            hi = min(n, lo + self.max_add)
            _lib.check(self.L.f110_replay_add(
                self.handle, ptr(s[lo:hi]), s.stride(0), ptr(a[lo:hi]), a.stride(0), ptr(r[lo:hi]), ptr(ns[lo:hi]),
                ns.stride(0), ptr(None if d is None else d[lo:hi]), ptr(None if pr is None else pr[lo:hi]),
                ptr(None if m is None else m[lo:hi]), hi - lo,
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
                self.handle, ptr(s[lo:hi]), s.stride(0), ptr(a[lo:hi]), a.stride(0), ptr(r[lo:hi]), ptr(ns[lo:hi]),
                ns.stride(0), ptr(d[lo:hi]), ptr(m[lo:hi]), hi - lo, self._stream()), "f110_replay_add_env")
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
            self.handle, B, float(beta), ptr(self.idx), ptr(self.weights),
            *((ptr(b["states"]), ptr(b["actions"]), ptr(b["rewards"]), ptr(b["next_states"]), ptr(b["dones"]))
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
        _lib.check(self.L.f110_replay_update_priorities(self.handle, ptr(i), ptr(t), i.shape[0], int(bool(td_errors)),
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
        _lib.check(self.L.f110_replay_select_keys(self.handle, ptr(k), k.shape[0], B, float(beta), ptr(self.idx),
                                                  ptr(self.weights), self._stream()), "f110_replay_select_keys")
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


class _EnvWindows:
    """What NStepAccumulator and ActionRepeat share: a library object of per-env state in front of a
    DeviceReplayBuffer (entry points f110_<KIND>_create / _destroy / _reset / _arrays), the checks
    of a step's reward and flag buffers, and the device copies of its arrays."""
    KIND = None  # "nstep" | "repeat"

    def __init__(self, n_envs, length, gamma, obs_dim, act_dim, device):
        self.L = _lib.load()
        self.n_envs, self.gamma = int(n_envs), float(gamma)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.handle = None
        self.device = dev = cuda_device(device, type(self).__name__)
        h = ctypes.c_void_p()
        _lib.check(self._entry("create")(ctypes.byref(h), dev.index or 0, self.n_envs, int(length), self.gamma,
                                         self.obs_dim, self.act_dim), f"f110_{self.KIND}_create")
        self.handle = h
        self._keep = self._keep_h = self._keep_m = None  # a call's inputs, alive until the stream has consumed them

    def _entry(self, name):
        return getattr(self.L, f"f110_{self.KIND}_{name}")

    def _stream(self):
        return stream(self.device)

    def _step_flags(self, rewards, terminated, truncated, was_reset, *rows):
        """push's reward and flag buffers as the simulator writes them, flat (truncated may be None);
        they and ``rows`` must have n_envs rows."""
        r, d, m = rewards.reshape(-1), terminated.reshape(-1), was_reset.reshape(-1)
        t = None if truncated is None else truncated.reshape(-1)
        if r.dtype != torch.float64 or d.dtype != torch.uint8 or m.dtype != torch.uint8 or \
                (t is not None and t.dtype != torch.uint8):
            raise TypeError("push: rewards float64, terminated, truncated and was_reset uint8")
        if not (r.is_contiguous() and d.is_contiguous() and m.is_contiguous() and (t is None or t.is_contiguous())):
            raise ValueError("push: contiguous rewards / flags")
        n = self.n_envs
        if any(x.shape[0] != n for x in (*rows, r, d, m)) or (t is not None and t.shape[0] != n):
            raise ValueError(f"push: every input needs n_envs = {n} rows")
        return r, d, t, m

    def reset(self, env_mask=None):
        """Drop the pending state of the envs with env_mask != 0 (None: all); nothing is emitted."""
        m = u8_rows(env_mask, None, self.device, "env_mask")
        if m is not None and m.shape[0] != self.n_envs:
            raise ValueError("reset: env_mask needs n_envs entries")
        self._keep_m = m
        _lib.check(self._entry("reset")(self.handle, ptr(m), self._stream()), f"f110_{self.KIND}_reset")

    def _copy_arrays(self, spec, first_only=False):
        """Device copies of the library's arrays: spec = (name, shape, dtype) in f110_<KIND>_arrays'
        order; first_only: the first array alone (the other pointers are not asked for)."""
        ptrs = [ctypes.c_void_p() for _ in spec[:1 if first_only else None]]
        _lib.check(self._entry("arrays")(self.handle, *[ctypes.byref(p) for p in ptrs],
                                         *[None] * (len(spec) - len(ptrs))), f"f110_{self.KIND}_arrays")
        out = {}
        for (name, shape, dt), p in zip(spec, ptrs):
            out[name] = torch.empty(shape, dtype=dt, device=self.device)
            _d2d(out[name], p.value, self._stream())
        return out

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self._entry("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NStepAccumulator(_EnvWindows):
    """N-step returns in front of a DeviceReplayBuffer (include/f110.h, "n-step returns"): per env a
    device window of at most ``n_step`` pending (s, a, running return) entries.  ``push`` takes a
    vector env's raw step outputs as ``add_env`` does and appends what leaves the windows to the
    ring: an entry with its n rewards, or every entry of an env whose episode ends.  A stored row's
    done column is the effective done 1 - gamma^(k-1) (1 - done), so the one-step learner
    bootstraps it with gamma^k.  ``reset`` drops the windows of the masked envs.  All on the current
    torch stream; nothing goes through the host."""
    KIND = "nstep"

    def __init__(self, n_envs: int, n_step: int, gamma: float, obs_dim: int = 1088, act_dim: int = 2, device=0):
        self.n_step = int(n_step)
        super().__init__(n_envs, n_step, gamma, obs_dim, act_dim, device)

    def push(self, memory: DeviceReplayBuffer, states, actions, rewards, next_states, terminated, truncated,
             was_reset):
        """One vector step into the windows; the emitted rows into ``memory``.  rewards float64,
        terminated / truncated / was_reset uint8 device tensors as the simulator writes them
        (truncated may be None: no episode limits); ``n_envs`` rows each."""
        s = memory._rows(states, self.obs_dim)
        ns = memory._rows(next_states, self.obs_dim)
        a = memory._rows(actions, self.act_dim)
        r, d, t, m = self._step_flags(rewards, terminated, truncated, was_reset, s, ns, a)
        self._keep = (s, ns, a, r, d, t, m)  # alive until the stream has consumed them
        _lib.check(self.L.f110_nstep_push(self.handle, memory.handle, ptr(s), s.stride(0), ptr(a), a.stride(0), ptr(r),
                                          ptr(ns), ns.stride(0), ptr(d), ptr(t), ptr(m), self._stream()),
                   "f110_nstep_push")
        memory.note_added(self.n_envs)  # an upper bound: emitted rows never outnumber pushed rows in total

    def _spec(self):
        N, n = self.n_envs, self.n_step
        return [("len", (N,), torch.int32), ("head", (N,), torch.int32), ("ret", (N, n), torch.float64),
                ("k", (N, n), torch.int32), ("obs", (N, n, self.obs_dim), torch.float32),
                ("act", (N, n, self.act_dim), torch.float32)]

    def arrays(self):
        """Device copies of the windows (tests): len, head [N] int32, ret [N, n] float64, k [N, n]
        int32, obs [N, n, D], act [N, n, A]; entry i of env e sits in slot (head + i) % n."""
        return self._copy_arrays(self._spec())

    def pending(self) -> torch.Tensor:
        """[n_envs] int32 copy of the window lengths."""
        return self._copy_arrays(self._spec(), first_only=True)["len"]


class ActionRepeat(_EnvWindows):
    """Action repeat around a vector env's step (include/f110.h, "action repeat"): per env a device
    phase, the block's first observation and action, and a running return.  ``hold`` runs before the
    env step: envs whose decision is due keep the policy's action and latch it with the observation;
    the others get their held action written over the policy's.  ``push`` runs after it and appends
    one row per finished block to the ring -- a block is finished after ``repeat`` steps or when its
    episode ends -- with the effective done 1 - gamma^(k-1) (1 - done), so the one-step learner
    bootstraps it with gamma^k.  ``reset`` drops the running blocks of the masked envs: a decision is
    due at their next hold.  All on the current torch stream; nothing goes through the host."""
    KIND = "repeat"

    def __init__(self, n_envs: int, repeat: int, gamma: float, obs_dim: int = 1088, act_dim: int = 2, device=0):
        self.repeat = int(repeat)
        super().__init__(n_envs, repeat, gamma, obs_dim, act_dim, device)
        self.decision = torch.zeros(self.n_envs, dtype=torch.uint8, device=self.device)  # written by the last hold

    def _rows(self, x, width, what):
        """x as [n_envs, width] float32 rows of unit inner stride, WITHOUT a copy (hold writes in
        place), and their row stride."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not same_device(x.device, self.device):
            raise TypeError(f"{what}: a float32 tensor on {self.device}")
        return f32_rows(x, self.n_envs, width, self.device, what, copy_ok=False)

    def hold(self, obs, act):
        """Before the env step.  obs [n_envs, obs_dim], act [n_envs, act_dim]: float32 device
        tensors or strided row views of them; act is rewritten in place and returned.
        ``decision`` [n_envs] uint8 is 1 where the policy's action was kept."""
        s, s_stride = self._rows(obs, self.obs_dim, "hold: obs")
        a, a_stride = self._rows(act, self.act_dim, "hold: act")
        self._keep_h = (s, a)  # alive until the stream has consumed them
        _lib.check(self.L.f110_repeat_hold(self.handle, ptr(s), s_stride, ptr(a), a_stride, ptr(self.decision),
                                           self._stream()), "f110_repeat_hold")
        return act

    def push(self, memory: DeviceReplayBuffer, rewards, next_obs, terminated, truncated, was_reset):
        """After the env step: one vector step into the blocks; the finished blocks into ``memory``.
        rewards float64, terminated / truncated / was_reset uint8 device tensors as the simulator
        writes them (truncated may be None: no episode limits); ``n_envs`` rows each."""
        ns = memory._rows(next_obs, self.obs_dim)
        r, d, t, m = self._step_flags(rewards, terminated, truncated, was_reset, ns)
        self._keep = (ns, r, d, t, m)  # alive until the stream has consumed them
        _lib.check(self.L.f110_repeat_push(self.handle, memory.handle, ptr(r), ptr(ns), ns.stride(0), ptr(d), ptr(t),
                                           ptr(m), self._stream()), "f110_repeat_push")
        memory.note_added(self.n_envs)  # an upper bound: at most one row per env and push

    def _spec(self):
        N = self.n_envs
        return [("k", (N,), torch.int32), ("ret", (N,), torch.float64), ("obs", (N, self.obs_dim), torch.float32),
                ("act", (N, self.act_dim), torch.float32)]

    def arrays(self):
        """Device copies of the state (tests): k [N] int32, ret [N] float64, obs [N, D], act [N, A]."""
        return self._copy_arrays(self._spec())

    def phase(self) -> torch.Tensor:
        """[n_envs] int32 copy of the phases (0: a decision is due)."""
        return self._copy_arrays(self._spec(), first_only=True)["k"]


def check_action_repeat(action_repeat) -> int:
    """action_repeat (a trainer's or a learner's argument) as an int: a ValueError unless it is an
    integer in 1..64."""
    import numpy as np
    if isinstance(action_repeat, bool) or not isinstance(action_repeat, (int, np.integer)) or \
            not 1 <= action_repeat <= 64:
        raise ValueError(f"action_repeat must be an integer in 1..64; got {action_repeat!r}")
    return int(action_repeat)


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
    _lib.check(L.f110_host_repeat_hold(N, D, A, *[ptr(x) for x in (state["k"], state["obs"], state["act"], obs, act,
                                                                   decision)]), "f110_host_repeat_hold")
    return act, decision


def _host_push_io(N, D, A, max_rows, reward, next_obs, terminated, truncated, was_reset):
    """A host push's step inputs as the C arrays the library reads, and the arrays it emits into:
    (reward, next_obs, flags, out rows (obs, act, reward, next_obs, done), the emitted-row count)."""
    import numpy as np
    next_obs = np.ascontiguousarray(next_obs, np.float32).reshape(N, D)
    reward = np.ascontiguousarray(reward, np.float64).reshape(N)
    flags = [None if f is None else np.ascontiguousarray(f, np.uint8).reshape(N)
             for f in (terminated, truncated, was_reset)]
    out = [np.empty((max_rows, D), np.float32), np.empty((max_rows, A), np.float32), np.empty(max_rows, np.float32),
           np.empty((max_rows, D), np.float32), np.empty(max_rows, np.float32)]
    return reward, next_obs, flags, out, ctypes.c_int64()


def host_repeat_push(state: dict, repeat, gamma, reward, next_obs, terminated, truncated, was_reset,
                     capacity: int = 0):
    """One push on the host (f110_host_repeat_push) over NumPy arrays.  Returns the emitted rows
    (obs, act, reward, next_obs, done) in the order the device appends them."""
    N, D = state["obs"].shape
    A = state["act"].shape[1]
    reward, next_obs, flags, out, cnt = _host_push_io(N, D, A, N, reward, next_obs, terminated, truncated, was_reset)
    _lib.check(_lib.load().f110_host_repeat_push(N, int(repeat), float(gamma), D, A, int(capacity),
                                                 *[ptr(state[q]) for q in ("k", "ret", "obs", "act")], ptr(reward),
                                                 ptr(next_obs), *[ptr(f) for f in flags], *[ptr(x) for x in out],
                                                 ctypes.byref(cnt)), "f110_host_repeat_push")
    return tuple(x[:cnt.value] for x in out)


def host_nstep(state: dict, gamma, obs, act, reward, next_obs, terminated, truncated, was_reset, capacity: int = 0):
    """One push on the host (f110_host_nstep) over NumPy arrays.  ``state``: the windows, as
    ``host_nstep_state`` makes them, updated in place.  Returns the emitted rows
    (obs, act, reward, next_obs, done) in the order the device appends them."""
    import numpy as np
    N, n = state["ret"].shape
    D, A = state["obs"].shape[2], state["act"].shape[2]
    obs = np.ascontiguousarray(obs, np.float32).reshape(N, D)
    act = np.ascontiguousarray(act, np.float32).reshape(N, A)
    reward, next_obs, flags, out, cnt = _host_push_io(N, D, A, N * n, reward, next_obs, terminated, truncated,
                                                      was_reset)
    _lib.check(_lib.load().f110_host_nstep(N, n, float(gamma), D, A, int(capacity),
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
