"""Action repeat on the host (no GPU): the new entry points are exported, and the host hooks
f110_host_repeat_hold / f110_host_repeat_push -- the per-env function the device kernel runs, over
host arrays -- equal the model of the rule written out in repeat_model.py bit for bit: the action
rows and decision mask of every hold, the emitted rows of every push and their order, the phases and
the running returns.  Every emitted row is also one of the n-step model's rows of the same push."""
import numpy as np
import pytest

from repeat_model import Model, RepeatModel, same_bits, scenario, stack_rows

T, N, D, A = 60, 7, 6, 2
NEW = ["f110_repeat_create", "f110_repeat_destroy", "f110_repeat_hold", "f110_repeat_push", "f110_repeat_reset",
       "f110_repeat_arrays", "f110_host_repeat_hold", "f110_host_repeat_push"]
ROW = ("obs", "act", "reward", "next_obs", "done")


@pytest.fixture(scope="module")
def sc():
    return scenario(T, N, D, A, seed=3)


def _flags(sc, t):
    return sc["rew"][t], sc["nxt"][t], sc["term"][t], sc["trunc"][t], sc["reset"][t]


def test_new_symbols_exported():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name


@pytest.mark.parametrize("gamma", [0.99, 0.5, 1.0, 0.0])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_host_hooks_equal_model(sc, K, gamma):
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_push, host_repeat_state
    st = host_repeat_state(N, D, A)
    model = RepeatModel(N, K, gamma)
    emitted = 0
    for t in range(T):
        want_a, want_d = model.hold(sc["obs"][t], sc["act"][t])
        got_a, got_d = host_repeat_hold(st, sc["obs"][t], sc["act"][t])
        assert same_bits(got_a, want_a) and np.array_equal(got_d, want_d) and got_d.dtype == np.uint8, t
        if K == 1:  # the hold changes nothing
            assert same_bits(got_a, sc["act"][t]) and got_d.all()
        want = stack_rows(model.push(*_flags(sc, t)), D, A)
        got = host_repeat_push(st, K, gamma, *_flags(sc, t))
        for name, g, w in zip(ROW, got, want):
            assert same_bits(g, w), f"{name}, push {t}"
        assert np.array_equal(st["k"], model.phases()), t
        assert same_bits(st["ret"], model.returns()), t
        assert (st["k"] <= K - 1).all()
        emitted += len(got[2])
        if K == 1:  # exactly f110_replay_add_env's rows
            keep = sc["reset"][t] == 0
            assert same_bits(got[0], sc["obs"][t][keep]) and same_bits(got[1], sc["act"][t][keep])
            assert same_bits(got[2], sc["rew"][t][keep].astype(np.float32))
            assert same_bits(got[3], sc["nxt"][t][keep])
            assert same_bits(got[4], sc["term"][t][keep].astype(np.float32))
    assert 0 < emitted <= int((sc["reset"] == 0).sum())
    if K == 1:
        assert emitted == int((sc["reset"] == 0).sum()) and model.held == 0


@pytest.mark.parametrize("seed", [3, 4])
@pytest.mark.parametrize("gamma", [0.99, 0.5, 1.0, 0.0])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_rows_are_nstep_rows(K, gamma, seed):
    """Model(N, K, gamma) fed the held actions emits, among the rows of each push, every row the
    host hook emits, in the same order: a block is the n-step entry that began at a decision step."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_push, host_repeat_state
    sc = scenario(T, N, D, A, seed=seed)
    st = host_repeat_state(N, D, A)
    nstep = Model(N, K, gamma)
    total = 0
    for t in range(T):
        act, _ = host_repeat_hold(st, sc["obs"][t], sc["act"][t])
        sup = stack_rows(nstep.push(sc["obs"][t], act, *_flags(sc, t)), D, A)
        got = host_repeat_push(st, K, gamma, *_flags(sc, t))
        j = 0
        for i in range(len(got[2])):
            while j < len(sup[2]) and not all(same_bits(g[i], s[j]) for g, s in zip(got, sup)):
                j += 1
            assert j < len(sup[2]), f"row {i} of push {t} is none of the n-step rows"
            j += 1
        total += len(got[2])
    assert total > 0


def test_scenario_covers_the_cases(sc):
    """K = 3 over the scenario: blocks that run to K, blocks ended by termination, by truncation
    alone, at least two blocks dropped by a reset row that met k > 0, and hold rows."""
    model = RepeatModel(N, 3, 0.99)
    for t in range(T):
        model.hold(sc["obs"][t], sc["act"][t])
        model.push(*_flags(sc, t))
    assert model.full > 0 and model.by_term > 0 and model.by_trunc > 0
    assert model.dropped >= 2 and model.held > 0


def test_negative_zero_reward_survives():
    """A lone -0.0 reward leaves as -0.0 (the block's return is assigned, not added to 0.0)."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_push, host_repeat_state
    st = host_repeat_state(1, D, A)
    z = np.zeros((1, D), np.float32)
    host_repeat_hold(st, z, np.zeros((1, A), np.float32))
    rows = host_repeat_push(st, 3, 0.99, np.array([-0.0]), z, [1], None, [0])
    assert len(rows[2]) == 1 and np.signbit(rows[2][0]) and rows[4][0] == 1.0


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=65), dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma=-0.1),
                                dict(capacity=N - 1), dict(n_envs=0)])
def test_argument_validation(kw):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_push, host_repeat_state
    n = kw.get("n_envs", N)
    st = host_repeat_state(n, D, A)
    args = (np.zeros(n), np.zeros((n, D), np.float32), np.zeros(n, np.uint8), None, np.zeros(n, np.uint8))
    with pytest.raises(_lib.F110Error, match="f110_host_repeat_push"):
        host_repeat_push(st, kw.get("K", 3), kw.get("gamma", 0.99), *args, capacity=kw.get("capacity", 0))


def test_hold_rejects_no_envs():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_state
    with pytest.raises(_lib.F110Error, match="f110_host_repeat_hold"):
        host_repeat_hold(host_repeat_state(0, D, A), np.zeros((0, D), np.float32), np.zeros((0, A), np.float32))


def test_valid_edges_pass():
    """repeat 1 and 64, gamma 0 and 1, n_envs == capacity."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_push, host_repeat_state
    args = (np.zeros(N), np.zeros((N, D), np.float32), np.zeros(N, np.uint8), None, np.zeros(N, np.uint8))
    for K, gamma in ((1, 0.0), (64, 1.0)):
        host_repeat_push(host_repeat_state(N, D, A), K, gamma, *args, capacity=N)


def test_learner_and_trainer_arguments():
    """ValueError before any network or env is built (no device needed)."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    from f110_gymnasium_ros2_jazzy_amd.train import ACTION_HIGH, ACTION_LOW, VectorTrainer
    kw = dict(obs_dim=1088, act_dim=2, action_low=ACTION_LOW, action_high=ACTION_HIGH)
    with pytest.raises(ValueError, match="n_step"):
        DDPGLearner(action_repeat=2, n_step=2, **kw)
    with pytest.raises(ValueError, match="action_repeat"):
        DDPGLearner(action_repeat=0, **kw)
    with pytest.raises(ValueError, match="action_repeat"):
        DDPGLearner(action_repeat=2.5, **kw)
    with pytest.raises(ValueError, match="device replay"):
        DDPGLearner(action_repeat=2, replay=None, **kw)
    with pytest.raises(ValueError, match="action_repeat"):
        VectorTrainer(64, action_repeat=65)
    with pytest.raises(ValueError, match="n_step"):
        VectorTrainer(64, action_repeat=2, n_step=2)
