"""Self-play, host side (no GPU): f110_host_agent_obs -- the statement of f110_agent_obs over host
arrays -- against the reference's recorded observations and a NumPy restatement bit for bit, its
argument errors, opponent.selfplay_mask, and the argument validation of F110VectorEnv and
VectorTrainer, which refuses a bad self-play argument before anything is built."""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LMAX = np.float32(30.0)


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def O():
    from f110_gymnasium_ros2_jazzy_amd import opponent
    return opponent


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def np_scan(s, lmax=LMAX):
    """F110Env._pack_flat_obs's scan entry (f110_env.py:557-560) in NumPy float32."""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(s, nan=lmax, posinf=lmax, neginf=0.0), np.float32(0), lmax) / np.float32(lmax)


def np_agent_obs(scans, obs, agent, lmax=LMAX):
    E, A, B = scans.shape
    order = [agent] + [i for i in range(A) if i != agent]
    pose = obs[:, B:B + 4 * A].reshape(E, A, 4)[:, order].reshape(E, 4 * A)
    return np.concatenate([np_scan(scans[:, agent], lmax), pose], axis=1)


def synthetic(E, A, B, seed=0):
    """Scans with every edge value (NaN, +-inf, negative, > lidar_max, 0, lidar_max, subnormals)
    spread over all agents, and an obs whose pose groups identify (env, agent, column)."""
    rng = np.random.default_rng(seed + 1000 * A + B)
    scans = rng.uniform(0.0, 31.0, (E, A, B)).astype(np.float32)
    edge = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0, 30.0, 30.000002, 45.0, 1e-45, -1e-45, 1.1754942e-38,
                     29.999998, 3.4e38], np.float32)
    flat = scans.reshape(-1)
    pos = rng.choice(flat.size, size=min(flat.size, 4 * edge.size * A), replace=False)
    flat[pos] = np.resize(edge, pos.size)
    obs = rng.uniform(-1.0, 1.0, (E, B + 4 * A)).astype(np.float32)
    obs[:, B:] = (np.arange(E)[:, None] * 100 + np.arange(4 * A)[None, :] + 0.25).astype(np.float32)
    return scans, obs


def test_exports(F):
    L = F.load()
    for n in ("f110_agent_obs", "f110_policy_head_rows", "f110_host_agent_obs"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION


@pytest.mark.parametrize("name", ["env_2agent.npz", "env_2agent_noise.npz", "env_gapfollow.npz"])
def test_reference_pin(O, name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        scans, obs = z["info_scans"], z["obs"]
    assert scans.dtype == np.float32 and obs.dtype == np.float32 and obs.shape[1] == 1088
    # the reference's own rows satisfy the NumPy statement (so the pin below is about the library)
    assert np.array_equal(bits(np_scan(scans[:, 0])), bits(obs[:, :1080]))
    got0 = O.host_agent_obs(scans, obs, 0, 30.0)
    assert np.array_equal(bits(got0), bits(obs))
    got1 = O.host_agent_obs(scans, obs, 1, 30.0)
    want1 = np.concatenate([np_scan(scans[:, 1]), obs[:, 1084:1088], obs[:, 1080:1084]], axis=1)
    assert np.array_equal(bits(got1), bits(want1))


@pytest.mark.parametrize("B", [1080, 37])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_edge_values(O, A, B):
    scans, obs = synthetic(3, A, B)
    assert np.isnan(scans).any() and np.isposinf(scans).any() and np.isneginf(scans).any()
    W = B + 4 * A
    for agent in range(A):
        want = np_agent_obs(scans, obs, agent)
        got = O.host_agent_obs(scans, obs, agent, 30.0)
        assert got.shape == (3, W) and np.array_equal(bits(got), bits(want)), (A, B, agent)
        # padded rows (the simulator's 1088-float stride for A = 1): the padding stays untouched
        pad = np.full((3, (W + 31) // 32 * 32 + 32), np.float32(-7.0))
        O.host_agent_obs(scans, obs, agent, 30.0, out=pad)
        assert np.array_equal(bits(pad[:, :W]), bits(want)) and (pad[:, W:] == -7.0).all()
    # agent 0 reproduces the input pose block
    assert np.array_equal(bits(O.host_agent_obs(scans, obs, 0, 30.0)[:, B:]), bits(obs[:, B:]))
    # another lidar_max than the default
    got = O.host_agent_obs(scans, obs, A - 1, 10.0)
    assert np.array_equal(bits(got), bits(np_agent_obs(scans, obs, A - 1, np.float32(10.0))))


def test_error_paths(F):
    L = F.load()
    E, A, B = 2, 2, 8
    W = B + 4 * A
    scans = np.zeros((E, A, B), np.float32)
    obs = np.zeros((E, W), np.float32)
    out = np.zeros((E, W), np.float32)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(scans_p=P(scans), ses=A * B, obs_p=P(obs), os_=W, n=E, a=A, b=B, agent=0, out_p=P(out), ost=W):
        return L.f110_host_agent_obs(scans_p, ses, obs_p, os_, n, a, b, agent, 30.0, out_p, ost)

    assert call() == 0
    bad = [dict(agent=-1), dict(agent=A), dict(ses=A * B - 1), dict(os_=W - 1), dict(ost=W - 1), dict(scans_p=None),
           dict(obs_p=None), dict(out_p=None), dict(n=0), dict(a=0), dict(b=0)]
    for kw in bad:
        assert call(**kw) == -1, kw  # F110_E_INVALID
        assert b"f110_host_agent_obs" in L.f110_last_error()
    # the device entry points refuse the same arguments before any device call
    null = ctypes.c_void_p(None)
    assert L.f110_agent_obs(P(scans), A * B, P(obs), W, E, A, B, A, 30.0, P(out), W, null) == -1
    assert b"f110_agent_obs" in L.f110_last_error()
    assert L.f110_agent_obs(P(scans), A * B, P(obs), W - 1, E, A, B, 0, 30.0, P(out), W, null) == -1
    assert L.f110_agent_obs(None, A * B, P(obs), W, E, A, B, 0, 30.0, P(out), W, null) == -1
    h = np.zeros((4, 128), np.float32)
    assert L.f110_policy_head_rows(P(h), P(h), P(h), P(h), P(h), 4, 128, 2, None, P(out), 1, null) == -1  # stride < nout
    assert b"f110_policy_head_rows" in L.f110_last_error()
    assert L.f110_policy_head_rows(P(h), None, P(h), P(h), P(h), 4, 128, 2, None, P(out), 4, null) == -1
    assert L.f110_policy_head_rows(P(h), P(h), P(h), P(h), P(h), 4, 128, 5, None, P(out), 8, null) == -1  # nout > 4


def test_selfplay_mask(O):
    full = O.selfplay_mask(4096, 0, 0.5)
    assert full.dtype == np.uint8 and full.shape == (4096,) and set(np.unique(full)) <= {0, 1}
    # independent of the sharding of [0, n)
    for cuts in ([0, 4096], [0, 1, 4096], [0, 1000, 1001, 2048, 4096], list(range(0, 4097, 512))):
        parts = [O.selfplay_mask(b - a, a, 0.5) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), full)
    assert not O.selfplay_mask(4096, 7, 0.0).any() and O.selfplay_mask(4096, 7, 1.0).all()
    assert 0.45 <= full.mean() <= 0.55
    # the rule itself, in Python integers
    g = 123456789
    for f in (0.25, 0.5, 0.9):
        assert O.selfplay_mask(1, g, f)[0] == int(((g * 2654435761) % 2**32) < f * 2**32)
    for f in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            O.selfplay_mask(4, 0, f)


class _FakePolicy:  # what F110VectorEnv checks of a PolicyOpponent on the host
    def __init__(self, n_envs, act_dim=2, lidar_max=30.0):
        self.n_envs, self.act_dim, self.lidar_max = n_envs, act_dim, lidar_max


def test_vector_env_argument_validation():
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    kw = dict(num_agents=2, device="cpu")  # nothing may be built: a build on this device would fail otherwise
    with pytest.raises(ValueError, match="'gap_follow', 'policy', 'mixed'"):
        F110VectorEnv(4, opponent="nonsense", **kw)
    with pytest.raises(ValueError, match="opponent_policy"):
        F110VectorEnv(4, opponent="policy", **kw)
    with pytest.raises(ValueError, match="opponent_policy"):
        F110VectorEnv(4, opponent="mixed", opponent_mask=np.zeros(4, np.uint8), **kw)
    with pytest.raises(ValueError, match="opponent_mask"):
        F110VectorEnv(4, opponent="mixed", opponent_policy=_FakePolicy(4), **kw)
    with pytest.raises(ValueError, match="opponent_mask"):
        F110VectorEnv(4, opponent="mixed", opponent_policy=_FakePolicy(4), opponent_mask=np.zeros(5, np.uint8), **kw)
    with pytest.raises(ValueError, match="opponent_mask"):
        F110VectorEnv(4, opponent="mixed", opponent_policy=_FakePolicy(4), opponent_mask=np.zeros(4, np.float32), **kw)
    with pytest.raises(ValueError, match="4 envs"):
        F110VectorEnv(4, opponent="policy", opponent_policy=_FakePolicy(5), **kw)
    with pytest.raises(ValueError, match="num_agents >= 2"):
        F110VectorEnv(4, num_agents=1, device="cpu", opponent="policy", opponent_policy=_FakePolicy(4))


def test_trainer_argument_validation():
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    for kw in (dict(selfplay_sync=0), dict(selfplay_sync=-3), dict(selfplay_sync=2.5), dict(selfplay_fraction=-0.01),
               dict(selfplay_fraction=1.01), dict(selfplay_fraction=float("nan")), dict(opponent="policy")):
        with pytest.raises(ValueError, match="selfplay_sync|selfplay_fraction|opponent"):
            VectorTrainer(4, opponent=kw.pop("opponent", "self"), device="cpu", **kw)
    with pytest.raises(ValueError, match="explicit learner path"):  # no explicit path on this device
        VectorTrainer(4, opponent="self", device="cpu")
