"""Shared by test_nstep_host.py and test_gpu_nstep.py: a NumPy model of the n-step window rule of
include/f110.h ("n-step returns"), written out independently of the library, the seeded step
sequences both tests push, and a NumPy ring that stores emitted rows the way one
f110_replay_add (priority NULL) of those rows does."""
import numpy as np

SPECIAL_REWARDS = (-0.0, 5e-324, 1e30)  # a negative zero, a denormal, a value whose sums overflow f32


def scenario(T, N, D, A, seed, isolated=((9, 1), (10, 1), (23, 3), (31, 0))):
    """T pushes of N envs: obs / next_obs [T, N, D] and act [T, N, A] f32, rewards [T, N] f64,
    terminated / truncated / was_reset [T, N] u8.  About one row in eight ends an episode:
    terminated, truncated or both; was_reset[t + 1] = terminated[t] | truncated[t] (NEXT_STEP
    autoreset) plus the isolated (t, env) rows, which mostly meet a non-empty window."""
    g = np.random.default_rng(seed)
    obs = g.standard_normal((T, N, D), dtype=np.float32)
    nxt = g.standard_normal((T, N, D), dtype=np.float32)
    act = g.standard_normal((T, N, A), dtype=np.float32)
    rew = g.standard_normal((T, N))
    for j, v in enumerate(SPECIAL_REWARDS * 4):
        rew[(3 * j + 1) % T, (5 * j + 2) % N] = v
    u = g.random((T, N))
    term = (u < 0.08).astype(np.uint8)
    trunc = ((u > 0.04) & (u < 0.12)).astype(np.uint8)  # 0.04 .. 0.08: both at once
    reset = np.zeros((T, N), np.uint8)
    for t in range(T):
        if t:
            reset[t] = term[t - 1] | trunc[t - 1]
        for ti, e in isolated:
            if ti == t and e < N:
                reset[t, e] = 1
        term[t][reset[t] != 0] = 0  # a reset row ends no episode
        trunc[t][reset[t] != 0] = 0
    return dict(obs=obs, act=act, rew=rew, nxt=nxt, term=term, trunc=trunc, reset=reset)


class Model:
    """The rule, one Python loop per env: a list of pending [s, a, ret, k] entries, returns as
    Python floats (IEEE doubles; a product and a sum are two roundings), the power table as
    sequential products."""

    def __init__(self, N, n, gamma):
        self.N, self.n = N, n
        self.pw = [1.0]
        for _ in range(n):
            self.pw.append(self.pw[-1] * float(gamma))
        self.win = [[] for _ in range(N)]

    def push(self, s, a, r, s2, term, trunc, reset):
        """Returns the emitted rows [(obs, act, reward f32, next_obs, done f32)], env ascending and
        oldest first within an env."""
        rows = []
        n, pw = self.n, self.pw
        with np.errstate(over="ignore"):
            for e in range(self.N):
                w = self.win[e]
                if reset[e]:
                    w.clear()
                    continue
                re = float(r[e])
                for ent in w:
                    p = pw[ent[3]] * re
                    ent[2] = ent[2] + p
                    ent[3] += 1
                w.append([s[e].copy(), a[e].copy(), re, 1])
                if term[e] or trunc[e]:
                    for ent in w:
                        d = np.float32(1.0) if term[e] else np.float32(1.0 - pw[ent[3] - 1])
                        rows.append((ent[0], ent[1], np.float32(ent[2]), s2[e], d))
                    w.clear()
                elif len(w) == n:
                    ent = w.pop(0)
                    rows.append((ent[0], ent[1], np.float32(ent[2]), s2[e], np.float32(1.0 - pw[n - 1])))
        return rows

    def lengths(self):
        return np.array([len(w) for w in self.win], np.int32)


def stack_rows(rows, D, A):
    """Model rows as the five arrays host_nstep returns."""
    m = len(rows)
    out = (np.empty((m, D), np.float32), np.empty((m, A), np.float32), np.empty(m, np.float32),
           np.empty((m, D), np.float32), np.empty(m, np.float32))
    for i, row in enumerate(rows):
        for dst, v in zip(out, row):
            dst[i] = v
    return out


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def live_entries(state):
    """(ret, k) of every pending entry of host / device windows, env by env, oldest first."""
    n = state["ret"].shape[1]
    ret, k = [], []
    for e, (ln, hd) in enumerate(zip(state["len"], state["head"])):
        for i in range(int(ln)):
            ret.append(state["ret"][e, (hd + i) % n])
            k.append(state["k"][e, (hd + i) % n])
    return np.array(ret, np.float64), np.array(k, np.int32)


class Ring:
    """The replay ring as NumPy arrays.  add(rows) stores them as one f110_replay_add with
    priority NULL does: consecutive slots from `next` (mod capacity), every row with the max
    priority over the first `length` slots taken before the add (1.0 when empty)."""
    NAMES = ("priority", "states", "actions", "rewards", "next_states", "dones")

    def __init__(self, cap, D, A):
        self.cap, self.length, self.next = cap, 0, 0
        self.a = {"priority": np.zeros(cap, np.float32), "states": np.zeros((cap, D), np.float32),
                  "actions": np.zeros((cap, A), np.float32), "rewards": np.zeros(cap, np.float32),
                  "next_states": np.zeros((cap, D), np.float32), "dones": np.zeros(cap, np.float32)}

    def add(self, obs, act, rew, nxt, done):
        m = len(rew)
        p0 = np.float32(self.a["priority"][:self.length].max()) if self.length else np.float32(1.0)
        slots = (self.next + np.arange(m)) % self.cap
        assert len(set(slots.tolist())) == m
        a = self.a
        a["priority"][slots] = p0
        a["states"][slots], a["actions"][slots], a["rewards"][slots] = obs, act, rew
        a["next_states"][slots], a["dones"][slots] = nxt, done
        self.length = min(self.length + m, self.cap)
        self.next = (self.next + m) % self.cap
