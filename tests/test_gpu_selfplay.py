"""Self-play on the device: f110_agent_obs against its host statement and against the simulator's own
obs rows, f110_policy_head_rows against the learner's actor head, F110VectorEnv's policy and mixed
opponents, and VectorTrainer(opponent="self"): the snapshot's sync, step graphs against the eager
loop, and the checkpoint's "opponent_actor"."""
import numpy as np
import pytest
import torch

from test_gpu_ddpg_heads import _close  # the explicit-vs-torch bar of the learner heads (rtol 1e-5)
from test_selfplay_host import bits, synthetic

pytestmark = pytest.mark.gpu

LOW, HIGH = [-0.4189, 0.0], [0.4189, 20.0]


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def dbits(t):
    return bits(t.detach().cpu().numpy())


@pytest.fixture(scope="module")
def O():
    from f110_gymnasium_ros2_jazzy_amd import opponent
    return opponent


def _learner(seed=3, obs_dim=1088):
    """A learner without a replay (its explicit path is the reference for the opponent's forward),
    with an output layer away from its near-zero init so that the actions vary over the rows."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    ln = DDPGLearner(obs_dim=obs_dim, act_dim=2, action_low=LOW, action_high=HIGH, seed=seed, device="cuda:0",
                     replay=None)
    assert ln.explicit is not None
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(seed)
        ln.actor.fc3.weight.copy_(torch.randn(2, 128, device="cuda", generator=g) * 0.2)
        ln.actor.fc3.bias.copy_(torch.randn(2, device="cuda", generator=g) * 0.1)
    return ln


# ---- 6: the kernel against the host statement -------------------------------------------------
@pytest.mark.parametrize("B", [1080, 37])
@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("E", [1, 5, 67])
def test_agent_obs_matches_host(gpu, O, E, A, B):
    scans, obs = synthetic(E, A, B, seed=E)
    W = B + 4 * A
    ds, do = torch.as_tensor(scans, device=gpu), torch.as_tensor(obs, device=gpu)
    for agent in range(A):
        want = bits(O.host_agent_obs(scans, obs, agent, 30.0))
        assert np.array_equal(dbits(O.agent_obs(ds, do, agent, 30.0)), want), (agent, "packed")
        # rows padded to the simulator's stride: the padding keeps its sentinel
        pad = torch.full((E, (W + 31) // 32 * 32 + 32), -7.0, device=gpu)
        O.agent_obs(ds, do, agent, 30.0, out=pad)
        assert np.array_equal(dbits(pad[:, :W]), want) and bool((pad[:, W:] == -7.0).all()), (agent, "padded")
    agent = A - 1
    want = bits(O.host_agent_obs(scans, obs, agent, 30.0))
    # out offset by one float: no 16-byte alignment, the 4-byte path, the same bits
    buf = torch.full((E * (W + 4) + 1,), -7.0, device=gpu)
    mis = buf[1:].view(E, W + 4)
    assert mis.data_ptr() % 16 == 4
    O.agent_obs(ds, do, agent, 30.0, out=mis)
    assert np.array_equal(dbits(mis[:, :W]), want) and float(buf[0]) == -7.0 and bool((mis[:, W:] == -7.0).all())
    # obs rows strided (a wider buffer's view)
    wide = torch.full((E, W + 40), 9.0, device=gpu)
    wide[:, :W] = do
    assert np.array_equal(dbits(O.agent_obs(ds, wide[:, :W], agent, 30.0)), want)
    with pytest.raises(ValueError):
        O.agent_obs(ds, do, A, 30.0)


# ---- 7: the simulator pins the kernel ---------------------------------------------------------
@pytest.mark.parametrize("E,A", [(33, 2), (22, 3)])
def test_agent_obs_reproduces_the_steps_obs(gpu, tracks, O, E, A):
    from f110_gymnasium_ros2_jazzy_amd.maps import centerline_spawns
    from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim
    sp = centerline_spawns("Spielberg", A)
    sim = BatchSim(tracks("Spielberg_map"), n_envs=E, n_agents=A, device=gpu, noise_std=0.01, seed=5)
    try:
        rng = np.random.default_rng(E)
        out = sim.reset(sp[rng.integers(0, sp.shape[0], E)])
        W = 1080 + 4 * A
        lmax = float(sim.params.lidar_max)
        g = torch.Generator(device=gpu).manual_seed(E)
        for t in range(4):
            if t:
                u = torch.rand(E, A, 2, device=gpu, generator=g)
                out = sim.step(u * torch.tensor([0.8378, 8.0], device=gpu) - torch.tensor([0.4189, 0.0], device=gpu))
            got = O.agent_obs(out.scans, out.obs, sim.cfg.ego_idx, lmax)
            assert same_bits(got, out.obs[:, :W]), f"step {t}"
            # the other seats: their own scan, their pose group first
            for agent in range(1, A):
                o = O.agent_obs(out.scans, out.obs, agent, lmax)
                assert same_bits(o[:, 1080:1084], out.obs[:, 1080 + 4 * agent:1084 + 4 * agent])
                assert same_bits(o[:, 1084:1088], out.obs[:, 1080:1084])
                assert bool((o[:, :1080] >= 0).all()) and bool((o[:, :1080] <= 1).all())
    finally:
        sim.close()


# ---- 8: the masked, strided head ------------------------------------------------------------
def test_policy_head_rows_matches_actor_head(gpu, O):
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import actor_head
    M, K, n = 70, 128, 2
    g = torch.Generator(device=gpu).manual_seed(8)
    h = torch.randn(M, K, device=gpu, generator=g)
    W = torch.randn(n, K, device=gpu, generator=g) * 0.2
    b = torch.randn(n, device=gpu, generator=g) * 0.1
    low, high = torch.tensor(LOW, device=gpu), torch.tensor(HIGH, device=gpu)
    scale, shift = 0.5 * (high - low), 0.5 * (high + low)
    with torch.no_grad():
        want = actor_head(h, W, b, scale, shift)
    assert want.shape == (M, n) and float(want.std()) > 0.1
    out = torch.full((M, n), -7.0, device=gpu)
    assert O.policy_head_rows(h, W, b, scale, shift, out) is out
    assert same_bits(out, want)
    # the [N, 2, 2] action buffer: the opponent's rows (stride 4), the other agent's columns stay
    act = torch.full((M, 2, 2), -7.0, device=gpu)
    O.policy_head_rows(h, W, b, scale, shift, act[:, 1])
    assert same_bits(act[:, 1], want) and bool((act[:, 0] == -7.0).all())
    mask = (torch.rand(M, device=gpu, generator=g) < 0.5).to(torch.uint8)
    assert 0 < int(mask.sum()) < M
    act.fill_(-7.0)
    O.policy_head_rows(h, W, b, scale, shift, act[:, 1], row_mask=mask)
    m = mask.bool()
    assert same_bits(act[:, 1][m], want[m]) and bool((act[:, 1][~m] == -7.0).all()) and bool((act[:, 0] == -7.0).all())
    act.fill_(-7.0)
    O.policy_head_rows(h, W, b, scale, shift, act[:, 1], row_mask=torch.zeros(M, dtype=torch.uint8, device=gpu))
    assert bool((act == -7.0).all())


# ---- 9: the env's policy and mixed opponents ---------------------------------------------------
def test_vector_env_policy_opponent(gpu, O, monkeypatch):
    import f110_gymnasium_ros2_jazzy_amd.ddpg as D
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    E = 33
    ln = _learner()
    opp = O.PolicyOpponent(ln.actor, E, gpu)
    assert same_bits(opp.flat, ln._flat["actor"]) and opp.flat.data_ptr() != ln._flat["actor"].data_ptr()
    assert opp.obs.shape == (E, 1088)
    ptrs = (opp.flat.data_ptr(), opp.obs.data_ptr())
    env = F110VectorEnv(E, num_agents=2, seed=7, device=gpu, opponent="policy", opponent_policy=opp)
    try:
        obs, infos = env.reset(seed=7)
        g = torch.Generator(device=gpu).manual_seed(9)
        for t in range(4):
            if t:
                u = torch.rand(E, 2, device=gpu, generator=g)
                obs, _, _, _, infos = env.step(u * torch.tensor([0.8378, 6.0], device=gpu) -
                                               torch.tensor([0.4189, 0.0], device=gpu))
            seat = O.agent_obs(env.sim.out.scans, obs, 1, 30.0)
            with torch.no_grad():
                want = ln.explicit.policy(ln.actor, seat)  # the same launches
                monkeypatch.setattr(D, "FUSED", False)
                ref = ln.actor(seat)  # the plain torch Actor
                monkeypatch.setattr(D, "FUSED", True)
            got = infos["opponent_actions"]
            assert same_bits(got, want), f"step {t}"
            assert float(got.std(0).min()) > 0  # the rows differ: a real forward, not a constant
            _close(got, ref, f"torch actor, step {t}")
            assert same_bits(env._act[:, 1], got)
        assert ptrs == (opp.flat.data_ptr(), opp.obs.data_ptr())
        # load: new weights, the same buffers
        with torch.no_grad():
            ln.actor.fc3.bias.add_(0.05)
        opp.load(ln.actor)
        assert same_bits(opp.flat, ln._flat["actor"]) and ptrs == (opp.flat.data_ptr(), opp.obs.data_ptr())
    finally:
        env.close()


def test_vector_env_mixed_opponent(gpu, O):
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    E = 33
    ln = _learner()
    opp = O.PolicyOpponent(ln.actor, E, gpu)
    mask = O.selfplay_mask(E, 0, 0.5)
    assert 0 < int(mask.sum()) < E
    m = torch.as_tensor(mask, device=gpu).bool()
    mixed = F110VectorEnv(E, num_agents=2, seed=7, device=gpu, opponent="mixed", opponent_policy=opp, opponent_mask=mask)
    rule = F110VectorEnv(E, num_agents=2, seed=7, device=gpu, opponent="gap_follow")
    try:
        obs, infos = mixed.reset(seed=7)
        _, infos_rule = rule.reset(seed=7)  # the same seed: both envs see the same scans at reset
        assert same_bits(mixed.sim.out.scans, rule.sim.out.scans)
        got = infos["opponent_actions"]
        assert same_bits(got[~m], infos_rule["opponent_actions"][~m])
        with torch.no_grad():
            want = ln.explicit.policy(ln.actor, O.agent_obs(mixed.sim.out.scans, obs, 1, 30.0))
        assert same_bits(got[m], want[m]) and not bool((got[m] == infos_rule["opponent_actions"][m]).all())
        g = torch.Generator(device=gpu).manual_seed(9)
        for t in range(3):  # the two envs part ways after the reset: each row kind against its own rule
            u = torch.rand(E, 2, device=gpu, generator=g)
            obs, _, _, _, infos = mixed.step(u * torch.tensor([0.8378, 6.0], device=gpu) -
                                             torch.tensor([0.4189, 0.0], device=gpu))
            got = infos["opponent_actions"]
            with torch.no_grad():
                want = ln.explicit.policy(ln.actor, O.agent_obs(mixed.sim.out.scans, obs, 1, 30.0))
            assert same_bits(got[m], want[m]), f"policy rows, step {t}"
            assert same_bits(got[~m], O.gap_follow(mixed.sim.out.scans[:, 1])[~m]), f"gap_follow rows, step {t}"
    finally:
        mixed.close()
        rule.close()


def test_policy_opponent_refuses_unsupported(O):
    from f110_gymnasium_ros2_jazzy_amd.ddpg import Actor
    with pytest.raises(ValueError):
        O.PolicyOpponent(Actor(12, 2, LOW, HIGH), 4, "cpu")
    with pytest.raises(ValueError):
        O.PolicyOpponent(Actor(12, 3, LOW + [0.0], HIGH + [1.0]), 4, "cuda:0")


# ---- 10: the trainer ---------------------------------------------------------------------------
STEPS = 14  # warm-up 4, then one update per step: 3 eager ones and 7 more


def _run_trainer(monkeypatch, flag, tmp_path=None):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    monkeypatch.setenv("F110_STEP_GRAPH", flag)
    tr = VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=4, seed=11, opponent="self", selfplay_sync=2)
    trace = []
    try:
        ag, opp = tr.agent, tr.opp
        assert opp is not None and tr.env.opponent == "policy" and ag.explicit is not None
        saved = {0: ag._flat["actor"].clone()}
        assert same_bits(opp.flat, saved[0])  # the snapshot starts as the initial actor
        for k in range(STEPS):
            tr.step()
            n = ag.global_step
            saved.setdefault(n, ag._flat["actor"].clone())
            assert same_bits(opp.flat, saved[n - n % 2]), f"step {k}: snapshot after {n} updates"
            if n % 2:
                assert not torch.equal(opp.flat, ag._flat["actor"]), f"step {k}: in between two syncs"
            trace.append((tr.obs.clone(), tr.env._act.clone(),
                          float(tr.last["critic_loss"]) if tr.last else None))
        torch.cuda.synchronize()
        assert ag.global_step == STEPS - 4 and ag._eager_left == 0
        assert ((0, True) in tr._sg and (1, True) in tr._sg) == (flag == "1")
        if tmp_path is not None:  # (c) the checkpoint carries the snapshot
            ag.path = str(tmp_path)
            tr.save_checkpoint("best.pt")
            ag.save_model("plain.pt")
            ck = torch.load(tmp_path / "best.pt", weights_only=True)
            plain = torch.load(tmp_path / "plain.pt", weights_only=True)
            assert set(ck) == set(plain) | {"opponent_actor"}
            assert set(ck["opponent_actor"]) == set(ag.actor.state_dict())
            snap, act = opp.flat.clone(), ag._flat["actor"].clone()
            ptr = opp.flat.data_ptr()
            opp.flat.zero_()
            assert tr.load_checkpoint("best.pt")
            assert same_bits(opp.flat, snap) and opp.flat.data_ptr() == ptr and same_bits(ag._flat["actor"], act)
            opp.flat.zero_()
            assert tr.load_checkpoint("plain.pt")  # no key: the snapshot stays as it is
            assert not bool(opp.flat.any())
    finally:
        tr.close()
    return trace


def test_trainer_selfplay_sync_graphs_and_checkpoint(gpu, monkeypatch, tmp_path):
    graphed = _run_trainer(monkeypatch, "1", tmp_path)
    eager = _run_trainer(monkeypatch, "0")
    assert len(graphed) == len(eager) == STEPS
    for k, ((o1, a1, l1), (o2, a2, l2)) in enumerate(zip(graphed, eager)):
        assert same_bits(o1, o2), f"obs, step {k}"
        assert same_bits(a1[:, 0], a2[:, 0]), f"ego actions, step {k}"
        assert same_bits(a1[:, 1], a2[:, 1]), f"opponent actions, step {k}"
        assert l1 == l2, f"critic loss, step {k}"
    assert graphed[-1][2] is not None
