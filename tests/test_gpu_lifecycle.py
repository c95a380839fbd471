"""Create / destroy of the four handle types on the GPU.  The contexts share one refcounted copy of a
map's EDT tables and every handle frees its device buffers through one allocator: a context that
goes must leave its neighbours on the same map untouched, and a handle created where another was
destroyed must compute what the first one did.  Nothing here looks at free memory (the card is shared).

straight_corridor, 3 envs x 2 agents, 64 beams; a ring of 8 rows, 2 envs x n = 2, a 2-point track."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E, A, B = 3, 2, 64


def _sim(tracks, gpu):
    from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim
    return BatchSim(tracks("straight_corridor"), n_envs=E, n_agents=A, num_beams=B, device=gpu, seed=11,
                    keep_f64_scans=True)


def _snap(sim):
    st, sb, sc = sim.get_state()
    o = sim.out
    return [x.cpu().numpy().copy() for x in (st, sb, sc, o.scans_f64, o.obs, o.collisions)]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), (what, i)


def test_contexts_share_a_map_and_part(tracks, gpu):
    """P and Q on one map; P allocates its lazy buffers (the per-env table, the ranges, the stall
    counters), both step twice, P closes.  Q's next two steps are bit for bit those of a fresh
    context R with the same seed and actions -- and so is a context built after the last one on the
    map has gone (the entry is freed and rebuilt)."""
    rng = np.random.default_rng(4)
    poses = np.array([[[10.0 + 6 * e, 0.3, 0.0], [12.5 + 6 * e, -0.4, 0.0]] for e in range(E)])
    acts = np.stack([rng.uniform(-0.3, 0.3, (4, E, A)), rng.uniform(1, 8, (4, E, A))], -1).astype(np.float32)
    P, Q = _sim(tracks, gpu), _sim(tracks, gpu)
    P.set_env_params({"mu": rng.uniform(0.7, 1.1, (E, A))})
    P.set_param_randomization({"mu": (0.6, 1.1)}, seed=3)
    P.set_episode_limits(stall_speed=0.5, stall_steps=3)
    for s in (P, Q):
        s.reset(poses)
        s.step(acts[0])
        s.step(acts[1])
    torch.cuda.synchronize()
    P.close()
    q = []
    for t in (2, 3):
        Q.step(acts[t])
        q.append(_snap(Q))
    R = _sim(tracks, gpu)
    R.reset(poses)
    first = None
    for t in range(4):
        R.step(acts[t])
        if t == 0:
            first = _snap(R)
        if t >= 2:
            _same(q[t - 2], _snap(R), f"step {t}")
    assert not np.array_equal(q[0][0], q[1][0])  # the cars do move
    Q.close()
    R.close()
    S = _sim(tracks, gpu)
    S.reset(poses)
    S.step(acts[0])
    _same(first, _snap(S), "rebuilt map entry")
    S.close()


def _replay_round(gpu):
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    g = torch.Generator().manual_seed(1)
    rows = [torch.rand(5, w, generator=g).to(gpu) for w in (8, 2, 1, 8)]
    rb = DeviceReplayBuffer(8, batch_size=4, obs_dim=8, act_dim=2, device=gpu, seed=5)
    try:
        rb.add(rows[0], rows[1], rows[2], rows[3], dones=torch.tensor([0, 1, 0, 0, 1]))
        idx, batch, w = rb.sample(beta=0.4)
        torch.cuda.synchronize()
        return [idx.cpu().numpy().copy(), w.cpu().numpy().copy()] + [batch[k].cpu().numpy().copy() for k in sorted(batch)] + \
               [len(rb)]
    finally:
        rb.close()


def _nstep_round(gpu):
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer, NStepAccumulator
    g = torch.Generator().manual_seed(2)
    obs, act, nxt = (torch.rand(2, w, generator=g).to(gpu) for w in (8, 2, 8))
    rew = torch.tensor([0.5, -1.25], dtype=torch.float64).to(gpu)
    term, reset = torch.tensor([1, 0], dtype=torch.uint8).to(gpu), torch.zeros(2, dtype=torch.uint8).to(gpu)
    rb = DeviceReplayBuffer(8, batch_size=4, obs_dim=8, act_dim=2, device=gpu, seed=5)
    acc = NStepAccumulator(2, 2, 0.99, obs_dim=8, act_dim=2, device=gpu)
    try:
        acc.push(rb, obs, act, rew, nxt, term, None, reset)
        win = acc.arrays()
        torch.cuda.synchronize()
        n = len(rb)
        assert n == 1 and acc.pending().tolist() == [0, 1]  # env 0's episode ended, env 1 waits for its 2nd reward
        return [win[k].cpu().numpy().copy() for k in ("len", "head", "ret", "k")] + \
               [win["obs"][1, 0].cpu().numpy().copy(), win["act"][1, 0].cpu().numpy().copy()] + \
               [v[:n].cpu().numpy().copy() for v in rb.arrays().values()]
    finally:
        acc.close()
        rb.close()


def _track_round(gpu):
    from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward, CenterlineTrack
    g = torch.Generator().manual_seed(3)
    obs = torch.rand(2, B + 8, generator=g).to(gpu)
    track = CenterlineTrack(np.array([[0.0, 0.0], [4.0, 1.0]]), closed=False, device=gpu)
    try:
        fn = BatchedCenterlineReward(2, 0.01, track, num_beams=B)
        r = [fn(obs).cpu().numpy().copy(), fn(obs).cpu().numpy().copy()]
        torch.cuda.synchronize()
        return r + [track.s.copy(), track.mid.copy(), np.float64(track.L)]
    finally:
        track.close()


@pytest.mark.parametrize("round_", [_replay_round, _nstep_round, _track_round], ids=["replay", "nstep", "track"])
def test_handle_created_again_computes_the_same(gpu, round_):
    """Create, one call, destroy; create again, the same call: equal results."""
    first, again = round_(gpu), round_(gpu)
    assert len(first) == len(again)
    for i, (x, y) in enumerate(zip(first, again)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), i
    assert any(np.asarray(x).any() for x in first)
