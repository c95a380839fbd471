"""The track observation on the device: f110_track_obs (k_track_obs) against its host statement on
the cases of test_track_obs_host.py, bit for bit; f110_ctx_track_obs on a BatchSim's live state;
F110VectorEnv(track_obs=True) beside a twin without it (eager steps, step_transition into a wide
buffer, one captured step); PolicyOpponent(track_obs=...); and VectorTrainer(track_obs=True) with
step graphs on and off."""
import numpy as np
import pytest
import torch

import pursuit_cases as C
import track_obs_cases as K

pytestmark = pytest.mark.gpu

B = 1080
TRACKS = ["spielberg", "open4", "triangle", "repeated", "cluster"]


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def TO():
    from f110_gymnasium_ros2_jazzy_amd import track_obs
    return track_obs


@pytest.fixture(scope="module")
def cases(gpu):
    """name -> (device CenterlineTrack, TrackOracle, poses float32 [M, 3]); built once."""
    import reward_oracle as R
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    out = {}
    xy, _, _ = C.spielberg_xy()
    named = {"spielberg": (xy, True), **C.small_tracks()}
    for name, (pts, closed) in named.items():
        T = R.TrackOracle(pts, closed=closed)
        tr = CenterlineTrack(pts, closed=closed, device=0)
        poses = np.concatenate([C.track_poses(T, lookahead=1.0, spread=3.0 if name == "spielberg" else 1.5),
                                C.special_poses()])
        out[name] = (tr, T, poses)
    yield out
    for tr, _, _ in out.values():
        tr.close()


def previews(name, n):
    scale = 1.0 if name == "spielberg" else 0.25
    return tuple(d * scale for d in K.PREVIEWS[n])


def host_tail(TO, track, sim, seat, other, **kw):
    """The host statement of the simulator's state as it is now."""
    st = sim.get_state()[0].cpu().numpy()
    return TO.host_track_obs(st, track, sim.E, sim.A, seat, other, **kw)


@pytest.mark.parametrize("name", TRACKS)
def test_kernel_matches_host(gpu, TO, cases, name):
    tr, T, poses = cases[name]
    n = 0
    for E in K.ENVS:
        for A, seat, other in K.SEATS:
            st = K.states_from_poses(poses, E, A, seed=n)  # (the pool holds non-finite poses too)
            dev = torch.as_tensor(st, device=gpu)
            for direction in (1, -1):
                for npv in (0, 4, 8):
                    kw = dict(preview=previews(name, npv), direction=direction)
                    want = TO.host_track_obs(st, tr, E, A, seat, other, **kw)
                    got = TO.track_obs(dev, tr, E, A, seat, other, **kw)
                    K.assert_rows_equal(got.cpu().numpy(), want, (name, E, A, seat, other, kw))
                    n += 1
    # the named corner cases of the host test, on the device: the seam, the clamp, the gap's wrap and clip
    rng = np.random.default_rng(3)
    s_at = np.concatenate([rng.uniform(0.0, 9.0, 16), T.L - rng.uniform(0.0, 9.0, 16), [0.0, T.L, 0.5 * T.L]])
    cars = []
    for s in s_at:
        i = T.seg_at(float(s))
        seg = T.s[i + 1] - T.s[i]
        p = T.xy[i] + (0.0 if seg == 0 else (s - T.s[i]) / seg) * (T.xy[i + 1] - T.xy[i])
        cars.append((np.float32(p[0]), np.float32(p[1]), np.float32(rng.uniform(-3.0, 3.0)), rng.uniform(-2.0, 9.0)))
    cars.append(cars[0])  # an even count: pairs (seat, other)
    st = K.state_of(cars)
    E = len(cars) // 2
    for kw in (dict(preview=previews(name, 4)), dict(preview=previews(name, 4), direction=-1, gap_scale=0.75)):
        want = TO.host_track_obs(st, tr, E, 2, 0, 1, **kw)
        got = TO.track_obs(torch.as_tensor(st, device=gpu), tr, E, 2, 0, 1, **kw)
        K.assert_rows_equal(got.cpu().numpy(), want, (name, "seam", kw))


def test_fallback_last_node_on_device(gpu, TO):
    """seg = n-1 from the nearest-node fallback (test_track_obs_host's track): the tangent index is
    clamped to n-2 on the device too."""
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    pts = np.array([[-50.0, 0.0]] + [[k * 1e-7, 0.0] for k in range(7)])
    tr = CenterlineTrack(pts, closed=False, device=0)
    try:
        st = K.state_of([(1.0, 0.0, 0.1, 2.0), (2.0, 0.5, 0.0, 1.0), (0.5, -0.25, 3.0, 1.0)])
        for kw in (dict(preview=(0.5, 20.0)), dict(preview=(0.5, 20.0), direction=-1)):
            want = TO.host_track_obs(st, tr, 1, 3, 0, 1, **kw)
            got = TO.track_obs(torch.as_tensor(st, device=gpu), tr, 1, 3, 0, 1, **kw)
            K.assert_rows_equal(got.cpu().numpy(), want, kw)
            assert np.isfinite(want).all() and abs(abs(want[0, 5]) - np.sin(0.1)) < 1e-6
    finally:
        tr.close()


def test_strided_rows_and_errors(gpu, TO, cases):
    tr, T, poses = cases["spielberg"]
    st = K.states_from_poses(poses, 7, 2, seed=3)
    dev = torch.as_tensor(st, device=gpu)
    want = TO.host_track_obs(st, tr, 7, 2, 1, 0)
    buf = torch.full((7, 11 + 20 + 6), -7.25, device=gpu)
    got = TO.track_obs(dev, tr, 7, 2, 1, 0, out=buf[:, 11:31])
    assert got.data_ptr() == buf[:, 11:31].data_ptr()
    K.assert_rows_equal(buf[:, 11:31].cpu().numpy(), want)
    assert bool((buf[:, :11] == -7.25).all()) and bool((buf[:, 31:] == -7.25).all())  # one writer per column, no more
    with pytest.raises(ValueError):
        TO.track_obs(dev, tr, 7, 2, 1, 0, out=buf[:, 11:30])
    with pytest.raises(ValueError):
        TO.track_obs(dev, tr, 7, 2, 1, 1)
    with pytest.raises(ValueError):
        TO.track_obs(dev[:, :13], tr, 7, 2)
    from f110_gymnasium_ros2_jazzy_amd._lib import F110Error
    with pytest.raises(F110Error, match="bad arguments"):
        TO.track_obs(dev, tr, 7, 2, 0, 1, preview=(1.0, 1e6))
    with pytest.raises(F110Error, match="bad arguments"):
        TO.track_obs(dev, tr, 7, 2, 0, 1, gap_scale=float("nan"))


def test_context_state(gpu, TO, cases, tracks):
    """f110_ctx_track_obs reads the simulator's live state: after set_state, and again after a step."""
    from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim
    tr, T, _ = cases["spielberg"]
    sim = BatchSim(tracks("Spielberg_map"), n_envs=3, n_agents=2, device=gpu, noise_std=0.0)
    try:
        k = np.array([[10, 40], [700, 650], [1500, 1560]]) % (T.n - 1)
        poses = np.concatenate([T.xy[k], np.arctan2(T.tan[k, 1], T.tan[k, 0])[..., None]], axis=2)
        sim.reset(poses)
        st = sim.get_state()[0].clone()
        rng = np.random.default_rng(0)
        st[2] = torch.as_tensor(rng.uniform(-0.3, 0.3, 6), device=gpu)    # delta
        st[3] = torch.as_tensor(rng.uniform(1.0, 8.0, 6), device=gpu)     # v
        st[5] = torch.as_tensor(rng.uniform(-2.0, 2.0, 6), device=gpu)    # yaw rate
        st[6] = torch.as_tensor(rng.uniform(-0.2, 0.2, 6), device=gpu)    # slip
        st[0] += torch.as_tensor(rng.uniform(-0.4, 0.4, 6), device=gpu)
        sim.set_state(st)
        for seat, other in ((0, 1), (1, 0), (1, None)):
            t = TO.TrackObs(sim, tr, seat=seat, other=other)
            assert t.width == (20 if other is not None else 16)
            wide = torch.full((3, B + 8 + t.width), 5.0, device=gpu)
            assert t.fill(wide[:, B + 8:]).data_ptr() == wide[:, B + 8:].data_ptr()
            want = host_tail(TO, tr, sim, seat, other)
            K.assert_rows_equal(wide[:, B + 8:].cpu().numpy(), want, (seat, other))
            assert bool((wide[:, :B + 8] == 5.0).all())
            # the library's own reading of the state, not a copy of it: the context-free entry on get_state
            K.assert_rows_equal(TO.track_obs(sim.get_state()[0], tr, 3, 2, seat, other).cpu().numpy(), want)
            assert float(np.abs(want[:, :4]).min()) > 0.0  # the dynamic state reached its columns
        t = TO.TrackObs(sim, tr, seat=0, other=1)
        out = torch.empty(3, t.width, device=gpu)
        before = t.fill(out).clone()
        sim.step(torch.tensor([[[0.1, 4.0], [-0.1, 3.0]]] * 3, device=gpu))
        t.fill(out)
        K.assert_rows_equal(out.cpu().numpy(), host_tail(TO, tr, sim, 0, 1), "after a step")
        assert not same_bits(out, before)
        with pytest.raises(ValueError):
            t.fill(torch.empty(3, t.width + 1, device=gpu))
        with pytest.raises(ValueError):
            TO.TrackObs(sim, tr, seat=2)
        with pytest.raises(ValueError):
            TO.TrackObs(sim, tr, seat=0, other=0)
        with pytest.raises(ValueError):
            TO.TrackObs(sim, tr, preview=(1e6,))
    finally:
        sim.close()


STEPS = 20


def _env(tr, wide, **kw):
    """Four two-agent envs racing the waypoint follower; wide: with the track observation."""
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    base = dict(num_agents=2, opponent="pure_pursuit", opponent_track=tr, opponent_speed=3.0, seed=5, device=0,
                max_episode_steps=7, infos="minimal")
    return F110VectorEnv(4, **{**base, **kw, **(dict(track_obs=True) if wide else {})})


def test_vector_env_beside_its_twin(gpu, TO, cases):
    """Same seed, same actions, 20 steps with a time limit of 7 (so every env autoresets twice): the
    left B + 8 columns, the rewards and the flags are the twin's bit for bit; the tail is the host
    statement of that step's state, the autoreset rows included; step_transition into a wide
    buffer gives the same rows."""
    tr, T, _ = cases["spielberg"]
    plain, wide, trans = _env(tr, False), _env(tr, True), _env(tr, True)
    trans_buf = torch.full((4, B + 8 + 20), float("nan"), device=gpu)
    try:
        W = B + 8
        assert wide.obs_dim == W + 20 == wide.single_observation_space.shape[0] and plain.obs_dim == W
        lo, hi = wide.single_observation_space.low, wide.single_observation_space.high
        assert np.array_equal(lo[:W], plain.single_observation_space.low)
        assert np.flatnonzero(np.isfinite(lo[W:])).tolist() == [5, 6, 15] and (hi[W:][[5, 6, 15]] == 1.0).all()
        o0, i0 = plain.reset(seed=9)
        o1, i1 = wide.reset(seed=9)
        o2, _ = trans.reset(seed=9)
        assert o1.shape == (4, W + 20) and same_bits(o1[:, :W], o0) and same_bits(o2, o1)
        assert set(i0) == set(i1)
        K.assert_rows_equal(o1[:, W:].cpu().numpy(), host_tail(TO, tr, wide.sim, 0, 1), "reset")
        rng = np.random.default_rng(1)
        resets = 0
        for k in range(STEPS):
            a = torch.as_tensor(np.stack([rng.uniform(-0.3, 0.3, 4), rng.uniform(1.0, 6.0, 4)], 1).astype(np.float32),
                                device=gpu)
            p_obs, p_rew, p_term, p_trunc, p_info = plain.step(a)
            w_obs, w_rew, w_term, w_trunc, w_info = wide.step(a)
            assert same_bits(w_obs[:, :W], p_obs), f"head, step {k}"
            assert torch.equal(w_rew.view(torch.int64), p_rew.view(torch.int64)), f"rewards, step {k}"
            assert torch.equal(w_term, p_term) and torch.equal(w_trunc, p_trunc), f"flags, step {k}"
            assert set(w_info) == set(p_info) and torch.equal(w_info["reset"], p_info["reset"])
            assert same_bits(w_info["opponent_actions"], p_info["opponent_actions"]), f"opponent, step {k}"
            K.assert_rows_equal(w_obs[:, W:].cpu().numpy(), host_tail(TO, tr, wide.sim, 0, 1), f"tail, step {k}")
            resets += int(w_info["reset"].sum())
            t_obs, t_rew, t_term, t_reset = trans.step_transition(a, obs_out=trans_buf)
            assert t_obs.data_ptr() == trans_buf.data_ptr() and same_bits(t_obs, w_obs), f"step_transition, step {k}"
            assert torch.equal(t_rew.view(torch.int64), w_rew.view(torch.int64)) and torch.equal(t_term.bool(), w_term)
        assert resets >= 8  # every env was reset on the device twice
        nxt = trans.step_transition(a)[0]  # without obs_out: a copy of the env's own wide rows
        assert nxt.shape == (4, W + 20) and nxt.data_ptr() != trans._wide.data_ptr() and same_bits(nxt, trans._wide)
        with pytest.raises(ValueError):
            trans.step_transition(a, obs_out=torch.empty(4, W, device=gpu))
    finally:
        for e in (plain, wide, trans):
            e.close()


def test_vector_env_single_agent(gpu, TO, cases):
    """One car per env: no gap columns (width 16), the centerline from obs_track, as_numpy observations."""
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    tr, T, _ = cases["spielberg"]
    env = F110VectorEnv(3, num_agents=1, seed=5, device=0, track_obs={"gap_scale": 4.0}, obs_track=tr, as_numpy=True)
    try:
        W = B + 4
        obs, _ = env.reset(seed=1)
        assert obs.shape == (3, W + 16) == (3, env.obs_dim) and env.single_observation_space.shape == (W + 16,)
        K.assert_rows_equal(obs[:, W:], host_tail(TO, tr, env.sim, 0, None))
        for k in range(3):
            obs = env.step(np.array([[0.1, 3.0]] * 3, np.float32))[0]
            K.assert_rows_equal(obs[:, W:], host_tail(TO, tr, env.sim, 0, None), k)
        assert (obs[:, W + 15] == 0.0).all() and (obs[:, W] > 0.0).all()  # the pad column; the speed column
    finally:
        env.close()


def test_vector_env_reward_and_race_read_wide_rows(gpu, TO, cases):
    """The reward and the race statistics on the wide rows give the twin's values."""
    from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward
    tr, T, _ = cases["spielberg"]
    envs = []
    try:
        for k in range(2):  # (a reward function holds per-env state: one each)
            rf = BatchedCenterlineReward(4, dt=0.01, progress=tr, device=gpu)
            envs.append(_env(tr, bool(k), race_stats=True, reward_fn=rf, opponent="gap_follow", opponent_track=None,
                             opponent_speed=None))
        plain, wide = envs
        assert wide._tobs.track is tr  # the centerline defaults to reward_fn.progress
        plain.reset(seed=2)
        wide.reset(seed=2)
        a = torch.tensor([[0.05, 5.0]] * 4, device=gpu)
        for k in range(12):
            p, w = plain.step(a), wide.step(a)
            assert torch.equal(w[1].view(torch.int64), p[1].view(torch.int64)), f"reward, step {k}"
            for key in ("progress", "lead", "result"):
                assert torch.equal(w[4]["race"][key], p[4]["race"][key]), (key, k)
        assert float(p[1].abs().sum()) > 0
    finally:
        for e in envs:
            e.close()


def test_captured_step_equals_eager(gpu, TO, cases):
    """One step_transition (simulator, tail, opponent) captured in a graph and replayed twice, on
    fixed action and observation buffers, against the same steps run eagerly."""
    tr, T, _ = cases["spielberg"]
    graphed, eager = _env(tr, True, max_episode_steps=2), _env(tr, True, max_episode_steps=2)
    try:
        graphed.reset(seed=4)
        eager.reset(seed=4)
        act = graphed.agent_actions()
        buf = torch.zeros(4, B + 8 + 20, device=gpu)
        acts = [torch.tensor([[0.02 * (k + 1), 3.0 + k]] * 4, device=gpu) for k in range(4)]
        want = []
        for a in acts:
            o, r, t, w = eager.step_transition(a)
            want.append((o.clone(), r.clone(), t.clone(), w.clone()))
        act.copy_(acts[0])
        got = [tuple(x.clone() for x in graphed.step_transition(act, obs_out=buf))]  # eager: loads every kernel
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.graph(g, stream=side):
            ret = graphed.step_transition(act, obs_out=buf)
        torch.cuda.current_stream(gpu).wait_stream(side)
        for a in acts[1:3]:
            act.copy_(a)
            g.replay()
            got.append(tuple(x.clone() for x in ret))
        act.copy_(acts[3])  # and eagerly again after the replays: the same buffers, the same state
        got.append(tuple(x.clone() for x in graphed.step_transition(act, obs_out=buf)))
        torch.cuda.synchronize()
        for k, (gk, wk) in enumerate(zip(got, want)):
            assert same_bits(gk[0], wk[0]), f"obs, step {k}"
            assert torch.equal(gk[1].view(torch.int64), wk[1].view(torch.int64)), f"rewards, step {k}"
            assert torch.equal(gk[2], wk[2]) and torch.equal(gk[3], wk[3]), f"flags, step {k}"
        assert int(sum(w[3].sum() for w in want)) >= 4  # an autoreset went through the captured step
        K.assert_rows_equal(buf[:, B + 8:].cpu().numpy(), host_tail(TO, tr, graphed.sim, 0, 1))
    finally:
        for e in (graphed, eager):
            e.close()


def test_policy_opponent_tail(gpu, TO, cases):
    from f110_gymnasium_ros2_jazzy_amd import opponent as O
    from f110_gymnasium_ros2_jazzy_amd.ddpg import Actor
    tr, T, _ = cases["spielberg"]
    env = _env(tr, True)
    try:
        env.reset(seed=3)
        env.step(torch.tensor([[0.1, 4.0]] * 4, device=gpu))
        W = B + 8
        torch.manual_seed(0)
        actor = Actor(W + 20, 2, [-0.4189, 0.0], [0.4189, 20.0]).to(gpu)
        seat = TO.TrackObs(env.sim, tr, seat=1, other=0)
        opp = O.PolicyOpponent(actor, 4, gpu, lidar_max=30.0, track_obs=seat)
        assert opp.obs_dim == W + 20 and opp.track_obs is seat
        rows = torch.zeros(4, 2, device=gpu)
        opp.act(env.sim.out, 1, rows, obs=env._wide)
        K.assert_rows_equal(opp.obs[:, W:].cpu().numpy(), host_tail(TO, tr, env.sim, 1, 0), "the opponent's seat")
        head = O.agent_obs(env.sim.out.scans, env._wide, 1, 30.0)
        assert same_bits(opp.obs[:, :W], head)
        assert bool(torch.isfinite(rows).all()) and float(rows.abs().sum()) > 0  # the forward ran on the wide rows
        # the ego's seat sees the gap with the other sign
        ego = host_tail(TO, tr, env.sim, 0, 1)
        assert np.allclose(ego[:, 15], -opp.obs[:, W + 15].cpu().numpy(), atol=1e-6)
        # an actor that takes the block and a snapshot without it: an error, not zeros
        bare = O.PolicyOpponent(actor, 4, gpu, lidar_max=30.0)
        with pytest.raises(ValueError, match="set_track_obs"):
            bare.act(env.sim.out, 1, rows, obs=env._wide)
        with pytest.raises(ValueError):
            bare.set_track_obs(TO.TrackObs(env.sim, tr, seat=1, other=0, preview=(1.0,)))
    finally:
        env.close()


TRAIN_STEPS = 12  # warm-up 4, then one update per step: 3 eager ones and 5 more


def _run_trainer(monkeypatch, flag, opponent):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    monkeypatch.setenv("F110_STEP_GRAPH", flag)
    tr = VectorTrainer(64, batch_size=64, memory_size=1024, warmup_steps=4, seed=11, opponent=opponent,
                       selfplay_sync=2, track_obs=True)
    try:
        ag = tr.agent
        assert ag.obs_dim == B + 8 + 20 == tr.env.obs_dim and tr.obs.shape == (64, B + 28)
        if opponent == "self":
            assert tr.opp.obs_dim == ag.obs_dim and tr.opp.track_obs.seat == 1 and tr.opp.track_obs.other == 0
        losses = []
        for _ in range(TRAIN_STEPS):
            tr.step()
            if tr.last:
                losses.append(float(tr.last["critic_loss"]))
        torch.cuda.synchronize()
        assert ag.global_step == TRAIN_STEPS - 4 >= 2 and len(losses) >= 2 and np.isfinite(losses).all()
        assert ((0, True) in tr._sg and (1, True) in tr._sg) == (flag == "1")
        tail = tr.obs[:, B + 8:]
        assert bool(torch.isfinite(tail).all()) and float(tail[:, 0].abs().max()) > 0  # the ego's speed column
        return ag._flat["actor"].clone(), tr.obs.clone(), losses
    finally:
        tr.close()


@pytest.mark.parametrize("opponent", ["gap_follow", "self"])
def test_trainer_track_obs(gpu, monkeypatch, opponent):
    """--track-obs through the trainer: the learner's obs_dim, finite losses, and step graphs that
    give the eager run's final actor weights bit for bit (the bar of the other step-graph tests)."""
    w1, o1, l1 = _run_trainer(monkeypatch, "1", opponent)
    w0, o0, l0 = _run_trainer(monkeypatch, "0", opponent)
    assert same_bits(o1, o0), "observations"
    assert l1 == l0, "critic losses"
    assert same_bits(w1, w0), "actor weights"


def test_trainer_arguments():
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    with pytest.raises(ValueError):
        VectorTrainer(64, track_preview=[1.0, 2.0])
    with pytest.raises(ValueError):
        VectorTrainer(64, track_obs=True, track_preview=[1.0] * 9)
    with pytest.raises(ValueError):
        VectorTrainer(64, track_obs=True, track_preview=[1.0, -2.0])
