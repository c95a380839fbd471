"""The pure-pursuit opponent on the device: f110_pure_pursuit (k_pursuit) against its host statement
on the tracks and poses of test_pursuit_host.py, its projection against the reward path's
(TrackOracle.project_xy), F110VectorEnv's "pure_pursuit" opponent step by step and over a lap's
worth of steps, the mixed opponent with the pure-pursuit rule, and VectorTrainer with step graphs
on and off."""
import numpy as np
import pytest
import torch

import pursuit_cases as C

pytestmark = pytest.mark.gpu

B = 1080


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def O():
    from f110_gymnasium_ros2_jazzy_amd import opponent
    return opponent


@pytest.fixture(scope="module")
def cases(gpu):
    """name -> (device CenterlineTrack, TrackOracle, poses float32 [M, 3]); built once."""
    import reward_oracle as R
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    out = {}
    xy, wr, wl = C.spielberg_xy()
    named = {"spielberg": (xy, True), **C.small_tracks()}
    for name, (pts, closed) in named.items():
        T = R.TrackOracle(pts, closed=closed)
        tr = CenterlineTrack(pts, closed=closed, device=0)
        poses = np.concatenate([C.track_poses(T, spread=3.0 if name == "spielberg" else 1.5), C.special_poses()])
        out[name] = (tr, T, poses)
    yield out
    for tr, _, _ in out.values():
        tr.close()


@pytest.mark.parametrize("name", ["spielberg", "open4", "triangle", "repeated", "cluster"])
def test_kernel_matches_host(gpu, O, cases, name):
    tr, T, poses = cases[name]
    la = 1.2 if name == "spielberg" else 1.0
    dev = torch.as_tensor(poses, device=gpu)
    for kw in (dict(lookahead=la), dict(lookahead=la, direction=-1), dict(lookahead=la, speed=2.5, steer_limit=0.05),
               dict(lookahead=la, a_lat=6.0, speed=12.0), dict(lookahead=la, a_lat=0.5, v_floor=1.5, speed=8.0)):
        want_a, want_x = O.host_pure_pursuit(poses, tr, return_aux=True, **kw)
        got_a, got_x = O.pure_pursuit(dev, tr, return_aux=True, **kw)
        C.assert_aux_equal(got_x.cpu().numpy(), want_x, (name, kw))
        C.assert_actions_close(got_a.cpu().numpy(), want_a, (name, kw))
    if name == "spielberg":  # the projection pin: what the reward path gives for the same points
        fin = np.isfinite(poses).all(axis=1)
        want = np.array([T.project_xy(float(p[0]), float(p[1])) for p in poses[fin]])
        C.assert_aux_equal(got_x.cpu().numpy()[fin, :2], want, "projection")


@pytest.mark.parametrize("M", C.ROWS + (130,))
def test_rows_strides_mask_speed(gpu, O, cases, M):
    tr, T, pool = cases["spielberg"]
    rng = np.random.default_rng(M)
    poses = pool[rng.integers(0, len(pool), M)]
    speeds = rng.uniform(0.0, 9.0, M)
    mask = (rng.random(M) < 0.5).astype(np.uint8)
    if M > 1:
        mask[-1], mask[0] = 0, 1  # the last row masked: with an odd M the tail half rides on a masked row
    want_a, want_x = O.host_pure_pursuit(poses, tr, row_speed=speeds, return_aux=True)
    # strided views: the pose group inside an obs tensor, the opponent's slot of an [M, A, 2] action buffer
    obs = torch.full((M, B + 8), 7.0, device=gpu)
    obs[:, B + 4:B + 7] = torch.as_tensor(poses, device=gpu)
    buf = torch.full((M, 2, 2), float("nan"), device=gpu)
    sp = torch.as_tensor(speeds, device=gpu)
    got, aux = O.pure_pursuit(obs[:, B + 4:B + 8], tr, out=buf[:, 1], row_speed=sp, return_aux=True)
    assert got.data_ptr() == buf[:, 1].data_ptr()
    C.assert_actions_close(buf[:, 1].cpu().numpy(), want_a, M)
    C.assert_aux_equal(aux.cpu().numpy(), want_x, M)
    assert bool(torch.isnan(buf[:, 0]).all())  # the ego's slots are untouched
    # masked rows keep their prior bytes: poisoned with NaN first, actions and aux
    from f110_gymnasium_ros2_jazzy_amd import _lib
    import ctypes
    poison_a = torch.full((M, 2), float("nan"), device=gpu)
    poison_x = torch.full((M, 4), float("nan"), dtype=torch.float64, device=gpu)
    dm = torch.as_tensor(mask, device=gpu)
    dp = torch.as_tensor(poses, device=gpu)
    p = O.pursuit_params()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = torch.cuda.current_stream(gpu).cuda_stream
    _lib.check(_lib.load().f110_pure_pursuit(tr.handle, ctypes.byref(p), vp(dp), M, 3, vp(sp), vp(dm), vp(poison_a), 2,
                                             vp(poison_x), ctypes.c_void_p(s)), "f110_pure_pursuit")
    pa, px = poison_a.cpu().numpy(), poison_x.cpu().numpy()
    keep = mask == 0
    assert np.isnan(pa[keep]).all() and np.isnan(px[keep]).all()
    C.assert_actions_close(pa[~keep], want_a[~keep], M)
    C.assert_aux_equal(px[~keep], want_x[~keep], M)
    # the Python wrapper's mask argument
    out2 = torch.full((M, 2), float("nan"), device=gpu)
    O.pure_pursuit(dp, tr, out=out2, row_mask=dm, row_speed=sp)
    assert same_bits(out2, poison_a)


def _env(gpu, track, n=64, **kw):
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    return F110VectorEnv(n, num_agents=2, seed=7, device=gpu, noise_std=0.0, opponent_track=track, **kw)


def test_vector_env_opponent_actions(gpu, O, cases):
    """infos["opponent_actions"] of every step is the host statement of the previous step's obs pose
    group: gap-follow's timing (the action a step applies was computed from the step before)."""
    tr = cases["spielberg"][0]
    speeds = np.linspace(2.0, 5.0, 64)
    env = _env(gpu, tr, opponent="pure_pursuit", opponent_params={"lookahead": 1.0}, opponent_speed=speeds)
    try:
        obs, infos = env.reset(seed=7)
        for t in range(200):
            prev = obs[:, B + 4:B + 7].cpu().numpy()
            want = O.host_pure_pursuit(prev, tr, row_speed=speeds, lookahead=1.0)
            C.assert_actions_close(infos["opponent_actions"].cpu().numpy(), want, f"step {t}")
            assert same_bits(env._act[:, 1], infos["opponent_actions"])
            ego = O.pure_pursuit(obs[:, B:B + 4], tr, speed=3.0)
            obs, _, _, _, infos = env.step(ego)
            if t == 0:
                applied = want
        assert float(np.abs(applied[:, 0]).max()) > 0 and np.array_equal(applied[:, 1], speeds.astype(np.float32))
    finally:
        env.close()


def test_vector_env_laps(gpu, O, cases):
    """64 envs from the closed-loop spawn layout, 1500 steps: the opponent on the env's own
    pure-pursuit launches, the ego through opponent.pure_pursuit on its pose group (library
    defaults for both).  No termination, progress >= 0.9 * 60 m, |t| <= 0.5 m."""
    tr, T, _ = cases["spielberg"]
    N, steps = 64, 1500
    env = _env(gpu, tr, n=N, opponent="pure_pursuit", infos="minimal")
    try:
        obs, _ = env.reset(options=C.lap_spawns(T, N).astype(np.float32))
        aux = torch.empty(steps, 2, N, 4, dtype=torch.float64, device=gpu)
        term = torch.zeros(N, dtype=torch.bool, device=gpu)
        for t in range(steps):
            ego, a0 = O.pure_pursuit(obs[:, B:B + 4], tr, return_aux=True)
            _, a1 = O.pure_pursuit(obs[:, B + 4:B + 8], tr, return_aux=True)
            aux[t, 0], aux[t, 1] = a0, a1
            obs, _, terminated, _, _ = env.step(ego)
            term |= terminated
        prog = C.Progress(T, 2 * N)
        for row in aux.reshape(steps, 2 * N, 4).cpu().numpy():
            prog.update(row)
        print(f"progress {prog.total.min():.3f} .. {prog.total.max():.3f} m, max |t| {prog.max_t:.4f} m, "
              f"terminated {int(term.sum())}")
        assert not bool(term.any())
        assert (prog.total >= 0.9 * 60.0).all()
        assert prog.max_t <= 0.5
    finally:
        env.close()


def test_vector_env_mixed_with_pursuit_rule(gpu, O, cases):
    from test_gpu_selfplay import _learner
    tr = cases["spielberg"][0]
    E = 33
    ln = _learner()
    mask = O.selfplay_mask(E, 0, 0.5)
    assert 0 < int(mask.sum()) < E
    m = torch.as_tensor(mask, device=gpu).bool()
    mixed = _env(gpu, tr, n=E, opponent="mixed", opponent_rule="pure_pursuit", opponent_mask=mask,
                 opponent_policy=O.PolicyOpponent(ln.actor, E, gpu))
    policy = _env(gpu, None, n=E, opponent="policy", opponent_policy=O.PolicyOpponent(ln.actor, E, gpu))
    rule = _env(gpu, tr, n=E, opponent="pure_pursuit")
    try:
        infos = [e.reset(seed=7)[1] for e in (mixed, policy, rule)]
        g = torch.Generator(device=gpu).manual_seed(9)
        for t in range(4):
            got, pol, pur = (i["opponent_actions"] for i in infos)
            assert same_bits(got[m], pol[m]), f"policy rows, step {t}"
            assert same_bits(got[~m], pur[~m]), f"pure-pursuit rows, step {t}"
            assert not bool((got[m] == pur[m]).all())
            u = torch.rand(E, 2, device=gpu, generator=g)
            a = u * torch.tensor([0.8378, 6.0], device=gpu) - torch.tensor([0.4189, 0.0], device=gpu)
            infos = [e.step(a)[4] for e in (mixed, policy, rule)]  # the rows are independent envs: each follows its kind
    finally:
        for e in (mixed, policy, rule):
            e.close()


STEPS = 12  # warm-up 4, then one update per step: 3 eager ones and 5 more


def _run_trainer(monkeypatch, flag):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    monkeypatch.setenv("F110_STEP_GRAPH", flag)
    tr = VectorTrainer(envs_per_rank=64, batch_size=64, memory_size=4096, warmup_steps=4, seed=11,
                       opponent="pure_pursuit", opponent_speed=3.5, opponent_lookahead=1.0)
    trace = []
    try:
        assert tr.env.opponent == "pure_pursuit" and tr.env.opponent_track is tr.track and tr.opp is None
        for _ in range(STEPS):
            rew, term = tr.step()
            trace.append((tr.env._act[:, 1].clone(), rew.clone(), term.clone()))
        torch.cuda.synchronize()
        assert ((0, True) in tr._sg and (1, True) in tr._sg) == (flag == "1")
    finally:
        tr.close()
    return trace


def test_trainer_step_graphs(gpu, monkeypatch):
    graphed = _run_trainer(monkeypatch, "1")
    eager = _run_trainer(monkeypatch, "0")
    assert len(graphed) == len(eager) == STEPS
    for k, ((a1, r1, t1), (a2, r2, t2)) in enumerate(zip(graphed, eager)):
        assert same_bits(a1, a2), f"opponent actions, step {k}"
        assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)), f"rewards, step {k}"
        assert torch.equal(t1, t2), f"terminated, step {k}"
    a = graphed[-1][0]
    assert bool((a[:, 1] == 3.5).all()) and float(a[:, 0].abs().max()) > 0  # the pursuit's rows, not zeros
