"""N-step returns on the host (no GPU): the new entry points are exported, and f110_host_nstep --
the per-env function the device kernel runs, over host arrays -- equals a NumPy model of the rule
written out in nstep_model.py bit for bit: emitted rows and their order, window lengths, running
returns and reward counts."""
import numpy as np
import pytest

from nstep_model import SPECIAL_REWARDS, Model, live_entries, same_bits, scenario, stack_rows

T, N, D, A = 60, 7, 6, 2
NEW = ["f110_nstep_create", "f110_nstep_destroy", "f110_nstep_push", "f110_nstep_reset", "f110_nstep_arrays",
       "f110_host_nstep"]


@pytest.fixture(scope="module")
def sc():
    return scenario(T, N, D, A, seed=3)


def test_new_symbols_exported():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_scenario_covers_the_cases(sc):
    """Termination, truncation, both at once and neither occur; -0.0, a denormal and 1e30 are pushed
    on rows that are no reset rows; some isolated reset rows exist."""
    te, tr, rs = sc["term"].astype(bool), sc["trunc"].astype(bool), sc["reset"].astype(bool)
    assert (te & ~tr).any() and (~te & tr).any() and (te & tr).any() and (~te & ~tr & ~rs).any()
    live = sc["rew"][~rs]
    assert (np.signbit(live) & (live == 0)).any() and (live == 5e-324).any() and (live == 1e30).any()
    prev_end = np.zeros_like(rs)
    prev_end[1:] = (te | tr)[:-1]
    assert (rs & ~prev_end).sum() >= 3 and (rs & prev_end).any()
    assert len(SPECIAL_REWARDS) == 3


@pytest.mark.parametrize("gamma", [0.99, 0.5, 1.0, 0.0])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_host_hook_equals_model(sc, n, gamma):
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    st = host_nstep_state(N, n, D, A)
    model = Model(N, n, gamma)
    emitted = frac = dropped = 0
    for t in range(T):
        step = (sc["obs"][t], sc["act"][t], sc["rew"][t], sc["nxt"][t], sc["term"][t], sc["trunc"][t],
                sc["reset"][t])
        before = model.lengths()
        dropped += int((before[sc["reset"][t] != 0] > 0).sum())
        want = stack_rows(model.push(*step), D, A)
        got = host_nstep(st, gamma, *step)
        for name, g, w in zip(("obs", "act", "reward", "next_obs", "done"), got, want):
            assert same_bits(g, w), f"{name}, push {t}"
        assert np.array_equal(st["len"], model.lengths()), t
        ret, k = live_entries(st)
        mret = np.array([ent[2] for w in model.win for ent in w], np.float64)
        mk = np.array([ent[3] for w in model.win for ent in w], np.int32)
        assert same_bits(ret, mret) and np.array_equal(k, mk), t
        assert (st["len"] <= n - 1).all() and (k <= n - 1).all()
        emitted += len(got[2])
        frac += int(((got[4] > 0) & (got[4] < 1)).sum())
        if n == 1:  # exactly f110_replay_add_env's rows
            keep = sc["reset"][t] == 0
            assert same_bits(got[0], sc["obs"][t][keep]) and same_bits(got[1], sc["act"][t][keep])
            assert same_bits(got[2], sc["rew"][t][keep].astype(np.float32))
            assert same_bits(got[3], sc["nxt"][t][keep])
            assert same_bits(got[4], sc["term"][t][keep].astype(np.float32))
    assert emitted > T * N // 2
    assert emitted <= int((sc["reset"] == 0).sum())  # never more rows out than pushed in
    if n > 1:
        assert dropped >= 2  # isolated reset rows met pending entries
        assert (frac > 0) == (0.0 < gamma < 1.0)


def test_negative_zero_reward_survives():
    """A lone -0.0 reward leaves as -0.0 (the new entry's return is assigned, not added to 0.0)."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    st = host_nstep_state(1, 3, D, A)
    z = np.zeros((1, D), np.float32)
    rows = host_nstep(st, 0.99, z, np.zeros((1, A), np.float32), np.array([-0.0]), z, [1], None, [0])
    assert len(rows[2]) == 1 and np.signbit(rows[2][0]) and rows[4][0] == 1.0


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=17), dict(gamma=1.5), dict(gamma=float("nan")),
                                dict(gamma=-0.1), dict(capacity=N * 3 - 1)])
def test_argument_validation(kw):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    n = kw.get("n", 3)
    st = host_nstep_state(N, n, D, A)
    z =np.zeros((N, D), np.float32)
    args = (z, np.zeros((N, A), np.float32), np.zeros(N), z, np.zeros(N, np.uint8), None, np.zeros(N, np.uint8))
    with pytest.raises(_lib.F110Error, match="f110_host_nstep"):
        host_nstep(st, kw.get("gamma", 0.99), *args, capacity=kw.get("capacity", 0))


def test_valid_edges_pass():
    """n_step 1 and 16, gamma 0 and 1, n_envs * n_step == capacity."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    z = np.zeros((N, D), np.float32)
    args = (z, np.zeros((N, A), np.float32), np.zeros(N), z, np.zeros(N, np.uint8), None, np.zeros(N, np.uint8))
    for n, gamma in ((1, 0.0), (16, 1.0)):
        host_nstep(host_nstep_state(N, n, D, A), gamma, *args, capacity=N * n)
