"""Episode limits and episode statistics, host side (no GPU): the new entry points are exported under
ABI 3, f110_set_episode_limits' validation refuses what it must (through its host hook: no context
can be created here), f110_host_episode_stats -- the device's per-env update and totals merge over
host arrays -- follows a plain NumPy statement of the semantics, and F110VectorEnv refuses bad
limits before it builds anything."""
import ctypes
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


def test_exports_and_abi(F):
    L = F.load()
    for n in ("f110_set_episode_limits", "f110_host_check_episode_limits", "f110_episode_scratch_bytes",
              "f110_episode_stats", "f110_host_episode_stats"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION
    assert ctypes.sizeof(F.F110EpisodeState) == 16 == F.EPISODE_STATE_BYTES
    assert ctypes.sizeof(F.F110EpisodeTotals) == 56 == F.EPISODE_TOTALS_BYTES
    assert L.f110_episode_scratch_bytes(1) > 0 and L.f110_episode_scratch_bytes(1000) >= L.f110_episode_scratch_bytes(1)


def _check(F, ms, sp, ss):
    L = F.load()
    rc = L.f110_host_check_episode_limits(ms, sp, ss)
    return rc, (L.f110_last_error() or b"").decode()


@pytest.mark.parametrize("args", [(0, 0.0, 0), (7, 0.0, 0), (0, 0.1, 5), (7, 0.1, 5)])
def test_limits_validation_accepts(F, args):
    assert _check(F, *args)[0] == 0


@pytest.mark.parametrize("args,name", [((-1, 0.0, 0), "max_steps"), ((0, 0.1, -5), "stall_steps"),
                                       ((0, -0.1, 5), "stall_speed"), ((0, float("nan"), 5), "stall_speed"),
                                       ((7, float("inf"), 0), "stall_speed")])
def test_limits_validation_refuses(F, args, name):
    rc, msg = _check(F, *args)
    assert rc == -1 and name in msg.split(":")[1]


# ---- f110_host_episode_stats against a NumPy model --------------------------------------------------
class Model:
    """The semantics of include/f110.h, one env at a time in plain Python."""

    def __init__(self, n):
        self.ret = np.zeros(n)
        self.len = np.zeros(n, np.int32)
        self.closed = np.zeros(n, np.int32)
        self.last_r = np.zeros(n)
        self.last_l = np.zeros(n, np.int32)
        self.fin = np.zeros(n, np.uint8)
        self.episodes = self.terminated = self.truncated = self.length_sum = 0
        self.returns = []  # every finished episode's return

    def update(self, r, term, trunc, wr):
        for e in range(len(r)):
            self.fin[e] = 0
            if wr[e]:
                self.ret[e], self.len[e], self.closed[e] = 0.0, 0, 0
            elif self.closed[e]:
                pass
            else:
                self.ret[e] += r[e]
                self.len[e] += 1
                if term[e] or (trunc is not None and trunc[e]):
                    self.fin[e] = 1
                    self.last_r[e], self.last_l[e] = self.ret[e], self.len[e]
                    self.closed[e] = 1
                    self.episodes += 1
                    self.terminated += int(bool(term[e]))
                    self.truncated += int(not term[e])
                    self.length_sum += int(self.len[e])
                    self.returns.append(float(self.ret[e]))


def _rows(rng, n, p_reset=0.05):
    """One call's inputs: rows with both flags set, and (p_reset small) closed envs that step on."""
    r = rng.normal(0.0, 3.0, n)
    term = (rng.random(n) < 0.08).astype(np.uint8)
    trunc = (rng.random(n) < 0.08).astype(np.uint8)
    both = rng.random(n) < 0.02
    term[both] = trunc[both] = 1
    wr = (rng.random(n) < p_reset).astype(np.uint8)
    return r, term, trunc, wr


def _state_fields(state):
    return (state[:, :8].copy().view(np.float64).ravel(), state[:, 8:12].copy().view(np.int32).ravel(),
            state[:, 12:16].copy().view(np.int32).ravel())


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("null_optional", [False, True])
def test_host_episode_stats_matches_model(F, n, null_optional):
    from f110_gymnasium_ros2_jazzy_amd.episode import host_episode_stats
    rng = np.random.default_rng(1000 * n + null_optional)
    state = np.zeros((n, 16), np.uint8)
    totals = F.F110EpisodeTotals()
    last_r, last_l, fin = (None, None, None) if null_optional else (np.zeros(n), np.zeros(n, np.int32),
                                                                   np.zeros(n, np.uint8))
    m = Model(n)
    abs_sum = 0.0
    saw_closed_step = saw_both = False
    for _ in range(50):
        r, term, trunc, wr = _rows(rng, n)
        saw_closed_step |= bool(np.any((m.closed == 1) & (wr == 0)))
        saw_both |= bool(np.any((term == 1) & (trunc == 1) & (wr == 0) & (m.closed == 0)))
        abs_sum += float(np.abs(r).sum())
        tr = None if null_optional else trunc
        host_episode_stats(r, term, tr, wr, state, last_r, last_l, fin, totals)
        m.update(r, term, tr, wr)
        ret, ln, closed = _state_fields(state)
        assert np.array_equal(ret, m.ret) and np.array_equal(ln, m.len) and np.array_equal(closed, m.closed)
        if not null_optional:
            assert np.array_equal(last_r, m.last_r) and np.array_equal(last_l, m.last_l)
            assert np.array_equal(fin, m.fin)
    if n > 1:
        assert saw_closed_step and (saw_both or null_optional or n < 1000)
    t = totals.as_dict()
    assert (t["episodes"], t["terminated"], t["truncated"], t["length_sum"]) == \
        (m.episodes, m.terminated, m.truncated, m.length_sum)
    if m.episodes:
        assert abs(t["return_sum"] - math.fsum(m.returns)) <= 1e-12 * abs_sum
        assert t["return_min"] == min(m.returns) and t["return_max"] == max(m.returns)
    if n > 1:
        assert m.episodes > 0 and m.terminated > 0
        assert null_optional or m.truncated > 0


def test_both_flags_count_as_terminated(F):
    from f110_gymnasium_ros2_jazzy_amd.episode import host_episode_stats
    state = np.zeros((3, 16), np.uint8)
    totals = F.F110EpisodeTotals()
    one = np.ones(3, np.uint8)
    host_episode_stats(np.array([1.0, 2.0, 3.0]), np.array([1, 0, 1], np.uint8), np.array([1, 1, 0], np.uint8),
                       np.zeros(3, np.uint8), state, totals=totals)
    t = totals.as_dict()
    assert (t["episodes"], t["terminated"], t["truncated"], t["length_sum"]) == (3, 2, 1, 3)
    assert (t["return_sum"], t["return_min"], t["return_max"]) == (6.0, 1.0, 3.0)
    # closed envs step on without a reset: ignored; then a reset row: ignored too, and a fresh episode
    host_episode_stats(np.array([9.0, 9.0, 9.0]), one, one, np.zeros(3, np.uint8), state, totals=totals)
    assert totals.episodes == 3
    host_episode_stats(np.array([9.0, 9.0, 9.0]), one, one, one, state, totals=totals)
    assert totals.episodes == 3 and not state.any()
    host_episode_stats(np.array([-4.0, 0.5, 0.5]), np.array([1, 0, 0], np.uint8), None, np.zeros(3, np.uint8), state,
                       totals=totals)
    t = totals.as_dict()
    assert (t["episodes"], t["terminated"], t["return_min"], t["return_sum"]) == (4, 3, -4.0, 2.0)


# ---- F110VectorEnv refuses bad limits before building anything ----------------------------------------
@pytest.mark.parametrize("kw,match", [(dict(max_episode_steps=-3), "max_steps"),
                                      (dict(stall_steps=5), "stall_speed"),
                                      (dict(stall_steps=5, stall_speed=0.0), "stall_speed"),
                                      (dict(stall_steps=-1, stall_speed=0.1), "stall_steps"),
                                      (dict(stall_steps=5, stall_speed=float("nan")), "stall_speed")])
def test_vector_env_refuses_bad_limits_before_building(kw, match):
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    with pytest.raises(ValueError, match=match):
        F110VectorEnv(4, map="straight_corridor", device="cpu", **kw)
