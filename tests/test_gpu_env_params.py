"""Per-env vehicle params and on-device domain randomization (f110_set_env_params,
f110_set_param_randomization; k_agents<., PENV>) on the GPU: a table's envs are bit for bit the
one-env contexts built with their params, the dynamics follow the oracle, the table-free path is
untouched, and the redraws at resets are keyed by (seed, global env id, agent, field, episode)
whatever the sharding, the stepping call (step, step_n, a captured graph) or the history."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIED = ("mu", "m", "C_Sf", "C_Sr", "a_max", "sv_max", "v_max")
CHOSEN = {70: (0, 1, 63, 64, 69), 33: (0, 1, 31, 32), 22: (0, 1, 20, 21)}  # both sides of the 64-car block edge
MU, M = (0.5, 1.25), (3.0, 4.5)


def _sim(tracks, gpu, track="Spielberg_map", **kw):
    from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim
    kw.setdefault("noise_std", 0.0)
    return BatchSim(tracks(track), device=gpu, **kw)


def _spawns(A=1):
    from f110_gymnasium_ros2_jazzy_amd.maps import centerline_spawns
    return centerline_spawns("Spielberg", A)


def _defaults():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    return _lib.default_params().as_dict()


def _draw_params(rng, E, A):
    d = _defaults()
    return {k: d[k] * rng.uniform(0.7, 1.2, (E, A)) for k in VARIED}


def _actions(rng, T, E, A):
    return np.stack([rng.uniform(-0.4189, 0.4189, (T, E, A)), rng.uniform(0, 20, (T, E, A))], -1).astype(np.float32)


def _snap(sim):
    st, sb, sc = sim.get_state()
    return st.cpu().numpy(), sb.cpu().numpy(), sc.cpu().numpy(), sim.out.scans_f64.cpu().numpy()


def _table(sim):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    p = sim.env_params()
    return np.stack([p[k] for k in _lib.PARAM_FIELDS], -1)  # [E, A, 19]


def _host_draw(seed, env, agent, episode, lo, hi):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    PP = ctypes.POINTER(_lib.F110Params)
    out = np.empty(19)
    rc = _lib.load().f110_host_param_draw(seed, env, agent, episode, lo.ctypes.data_as(PP), hi.ctypes.data_as(PP),
                                          out.ctypes.data_as(PP))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def table_run_a1(tracks, gpu):
    """E = 70, A = 1 (two blocks, 58 padding lanes), RK4: the per-env params, the poses, the actions
    and the trajectory of the table context -- computed once, read by the tests below."""
    E, A, T = 70, 1, 40
    rng = np.random.default_rng(2024)
    sp = _spawns(A)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    params = _draw_params(rng, E, A)
    acts = _actions(rng, T, E, A)
    sim = _sim(tracks, gpu, n_envs=E, n_agents=A, keep_f64_scans=True)
    sim.set_env_params(params)
    sim.reset(poses)
    traj = [_snap(sim)]
    cols = []
    for t in range(T):
        cols.append(sim.step(acts[t]).collisions.cpu().numpy())
        traj.append(_snap(sim))
    sim.close()
    return dict(E=E, A=A, T=T, poses=poses, params=params, acts=acts, traj=traj, cols=np.array(cols))


def _check_against_one_env_contexts(tracks, gpu, E, A, poses, params, acts, traj, **kw):
    for e in CHOSEN[E]:
        ref = _sim(tracks, gpu, n_envs=1, n_agents=A, keep_f64_scans=True, env_offset=e,
                   params={k: v[e, 0] for k, v in params.items()}, **kw)
        for i in range(1, A):  # RaceCar i's own params (Simulator.update_params(params, index))
            ref.update_params({k: v[e, i] for k, v in params.items()}, agent_idx=i)
        ref.reset(poses[e:e + 1])
        for t in range(len(acts) + 1):
            if t:
                ref.step(acts[t - 1, e:e + 1])
            g = slice(e * A, (e + 1) * A)
            st, sb, sc, scans = _snap(ref)
            assert np.array_equal(traj[t][0][:, g], st), (e, t)
            assert np.array_equal(traj[t][1][:, g], sb), (e, t)
            assert np.array_equal(traj[t][2][g], sc), (e, t)
            assert np.array_equal(traj[t][3][e], scans[0]), (e, t)
        ref.close()


def test_table_matches_one_env_contexts_a1(tracks, gpu, table_run_a1):
    r = table_run_a1
    assert len({tuple(r["traj"][-1][0][:, e]) for e in range(r["E"])}) == r["E"]  # the envs do differ
    _check_against_one_env_contexts(tracks, gpu, r["E"], r["A"], r["poses"], r["params"], r["acts"], r["traj"])


@pytest.mark.parametrize("E,A,integrator", [(33, 2, 1), (22, 3, 1), (70, 1, 2)])
def test_table_matches_one_env_contexts(tracks, gpu, E, A, integrator):
    """66 cars with hand-off masks (k_agents<true, true>), 66 without (A = 3), and Euler; the
    agents of one env have different rows."""
    T = 40
    rng = np.random.default_rng(100 * A + integrator)
    sp = _spawns(A)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    params = _draw_params(rng, E, A)
    acts = _actions(rng, T, E, A)
    sim = _sim(tracks, gpu, n_envs=E, n_agents=A, keep_f64_scans=True, integrator=integrator)
    sim.set_env_params(params)
    got = sim.env_params()
    for k in VARIED:
        assert np.array_equal(got[k], params[k])
    sim.reset(poses)
    traj = [_snap(sim)]
    for t in range(T):
        sim.step(acts[t])
        traj.append(_snap(sim))
    sim.close()
    _check_against_one_env_contexts(tracks, gpu, E, A, poses, params, acts, traj, integrator=integrator)


def test_table_dynamics_vs_oracle(table_run_a1, oracle_mod):
    """Each env's states against oracle.update_pose under that env's Params, free-running over the
    same actions, at test_gpu_parity.py's RK4 trace tolerance (rtol = atol = 1e-12)."""
    O = oracle_mod
    r = table_run_a1
    assert not r["cols"].any()  # no TTC response in the run: update_pose alone is the whole state update
    for e in range(r["E"]):
        P = O.make_params({k: float(v[e, 0]) for k, v in r["params"].items()})
        st = np.zeros(7)
        st[0], st[1], st[4] = r["poses"][e, 0]
        buf, cnt = np.zeros(2), np.zeros(1, np.int32)
        O.update_pose(st, buf, cnt, 0.0, 0.0, P)  # F110Env.reset's zero-action step
        np.testing.assert_allclose(r["traj"][0][0][:, e], st, rtol=1e-12, atol=1e-12)
        for t in range(r["T"]):
            O.update_pose(st, buf, cnt, float(r["acts"][t, e, 0, 0]), float(r["acts"][t, e, 0, 1]), P)
            np.testing.assert_allclose(r["traj"][t + 1][0][:, e], st, rtol=1e-12, atol=1e-12, err_msg=f"env {e} step {t}")


def test_default_path_untouched(tracks, gpu):
    E, A = 70, 1
    rng = np.random.default_rng(5)
    sp = _spawns(A)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    acts = _actions(rng, 20, E, A)
    never = _sim(tracks, gpu, n_envs=E, n_agents=A, keep_f64_scans=True)
    dropped = _sim(tracks, gpu, n_envs=E, n_agents=A, keep_f64_scans=True)
    dropped.set_env_params(_draw_params(rng, E, A))
    dropped.set_env_params(None)
    d = _defaults()
    for sim in (never, dropped):
        p = sim.env_params()
        assert set(p) == set(d)
        for k, v in p.items():
            assert v.shape == (E, A) and v.dtype == np.float64 and (v == d[k]).all(), k
        sim.reset(poses)
        for t in range(20):
            sim.step(acts[t])
    for a, b in zip(_snap(never), _snap(dropped)):
        assert np.array_equal(a, b)
    # update_params still reaches the table-free dynamics, and env_params shows it
    never.update_params({"mu": 0.7})
    assert (never.env_params()["mu"] == 0.7).all()
    never.close()
    dropped.close()


def test_set_env_params_validation(tracks, gpu):
    from f110_gymnasium_ros2_jazzy_amd._lib import F110Error
    E = 6
    sim = _sim(tracks, gpu, n_envs=E, n_agents=1)
    mu = np.linspace(0.6, 1.1, E)
    sim.set_env_params({"mu": mu})
    before = _table(sim)
    length = np.full(E, _defaults()["length"])
    length[4] = 0.7
    with pytest.raises(F110Error, match="length"):
        sim.set_env_params({"mu": mu[::-1].copy(), "length": length})
    with pytest.raises(F110Error, match="C_Sr"):
        sim.set_env_params({"C_Sr": np.array([1.0, np.nan, 1.0, 1.0, 1.0, 1.0])})
    with pytest.raises(F110Error, match="lidar_max"):
        sim.set_param_randomization({"lidar_max": (10.0, 30.0)})
    with pytest.raises(ValueError, match="nope"):
        sim.set_env_params({"nope": 1.0})
    assert np.array_equal(_table(sim), before) and np.array_equal(before[:, 0, 0], mu)
    sim.close()


def test_randomization_properties(tracks, gpu):
    E, A = 4096, 1
    sp = _spawns(A)
    poses = sp[np.random.default_rng(3).integers(0, sp.shape[0], E)]
    d = _defaults()

    def table(seed, rseed, sim_out=None):
        sim = _sim(tracks, gpu, n_envs=E, n_agents=A, seed=seed)
        sim.set_param_randomization({"mu": MU, "m": M}, seed=rseed)
        sim.reset(poses)
        t = sim.env_params()
        if sim_out is not None:
            sim_out.append(sim)
        else:
            sim.close()
        return t

    keep = []
    t0 = table(42, 7, keep)
    mu, m = t0["mu"][:, 0], t0["m"][:, 0]
    assert (mu >= MU[0]).all() and (mu < MU[1]).all() and (m >= M[0]).all() and (m < M[1]).all()
    for k, v in t0.items():
        if k not in ("mu", "m"):
            assert (v == d[k]).all(), k
    assert len(np.unique(mu)) > 4000
    se = (MU[1] - MU[0]) / np.sqrt(12.0 * E)  # the uniform law's standard error of the mean
    print(f"mean(mu) - midpoint = {mu.mean() - 0.5 * (MU[0] + MU[1]):+.3e}, standard error {se:.3e}")
    assert abs(mu.mean() - 0.5 * (MU[0] + MU[1])) < 5 * se
    t1 = table(42, 7)
    assert all(np.array_equal(t0[k], t1[k]) for k in t0)        # same seeds, same cars
    t2 = table(42, 8)
    assert not np.array_equal(t0["mu"], t2["mu"]) and not np.array_equal(t0["m"], t2["m"])
    # an explicit reset reproduces the cars, whatever ran in between
    sim = keep[0]
    sim.step(np.zeros((E, A, 2), np.float32))
    sim.reset(poses)
    t3 = sim.env_params()
    assert all(np.array_equal(t0[k], t3[k]) for k in t0)
    # seed=None is the context's seed
    sim.set_param_randomization({"mu": MU, "m": M})
    sim.reset(poses)
    assert not np.array_equal(sim.env_params()["mu"], t0["mu"])
    t42 = table(5, 42)
    assert np.array_equal(sim.env_params()["mu"], t42["mu"])
    # and the device draws what the header describes (the host copy of the draw)
    from f110_gymnasium_ros2_jazzy_amd.sim import param_range_rows
    lo, hi = param_range_rows({"mu": MU, "m": M}, [d])
    for e in (0, 1, 63, 64, 4095):
        assert np.array_equal(_host_draw(7, e, 0, 0, lo[0], hi[0])[:16], np.array([t0[k][e, 0] for k in list(t0)[:16]]))
    sim.close()


def test_shard_invariance(tracks, gpu):
    """8 envs in one context = two 4-env contexts at env_offset 0 and 4 = StreamShards with 2 streams."""
    from f110_gymnasium_ros2_jazzy_amd.streams import StreamShards
    E, A, T = 8, 1, 30
    rng = np.random.default_rng(8)
    sp = _spawns(A)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    acts = _actions(rng, T, E, A)
    ranges = {"mu": MU, "m": M, "a_max": (6.0, 11.0)}
    full = _sim(tracks, gpu, n_envs=E, n_agents=A, seed=3)
    halves = [_sim(tracks, gpu, n_envs=E // 2, n_agents=A, seed=3, env_offset=4 * h) for h in range(2)]
    shards = StreamShards(tracks("Spielberg_map"), n_envs=E, n_streams=2, n_agents=A, seed=3, noise_std=0.0, device=gpu)
    for s in [full, shards] + halves:
        s.set_param_randomization(ranges, seed=11)
    full.reset(poses)
    shards.reset(poses)
    for h in range(2):
        halves[h].reset(poses[4 * h:4 * h + 4])
    tf = _table(full)
    assert len(np.unique(tf[:, 0, 0])) == E
    assert np.array_equal(tf, np.concatenate([_table(h) for h in halves]))
    assert all(np.array_equal(v, full.env_params()[k]) for k, v in shards.env_params().items())
    for t in range(T):
        full.step(acts[t])
        shards.step(acts[t])
        for h in range(2):
            halves[h].step(acts[t, 4 * h:4 * h + 4])
    shards.join()
    sf = full.get_state()[0].cpu().numpy()
    assert np.array_equal(sf, np.concatenate([h.get_state()[0].cpu().numpy() for h in halves], 1))
    assert np.array_equal(sf, np.concatenate([sm.get_state()[0].cpu().numpy() for sm in shards.sims], 1))
    # StreamShards.set_env_params splits the rows over the sub-shards
    mu = np.linspace(0.6, 1.1, E)
    shards.set_env_params({"mu": mu, "m": 3.5})
    p = shards.env_params()
    assert np.array_equal(p["mu"][:, 0], mu) and (p["m"] == 3.5).all()
    assert np.array_equal(shards.sims[1].env_params()["mu"][:, 0], mu[4:])
    for s in [full, shards] + halves:
        s.close()


def test_masked_reset_redraws_only_its_envs(tracks, gpu):
    E, A = 16, 1
    sp = _spawns(A)
    poses = sp[::300][:E]
    sim = _sim(tracks, gpu, n_envs=E, n_agents=A)
    sim.set_param_randomization({"mu": MU, "m": M}, seed=1)
    sim.reset(poses)
    t0 = _table(sim)
    sim.set_param_randomization({"mu": (2.0, 3.0), "m": M}, seed=1)  # (so that a redrawn row shows)
    mask = np.zeros(E, np.uint8)
    mask[[2, 7, 13]] = 1
    sim.reset(poses, env_mask=mask)
    t1 = _table(sim)
    changed = np.any(t1 != t0, axis=(1, 2))
    assert np.array_equal(changed, mask.astype(bool))
    assert (t1[mask == 1, 0, 0] >= 2.0).all() and np.array_equal(t1[mask == 1, 0, 6], t0[mask == 1, 0, 6])  # m: same draw
    # randomization off: the table stays as it stands, and resets leave it alone
    sim.set_param_randomization(None)
    sim.reset(poses)
    assert np.array_equal(_table(sim), t1)
    sim.close()


def test_autoreset_redraws_by_episode(tracks, gpu):
    """straight_corridor, every car driven into the wall 1 m ahead, autoreset on: the step that resets
    env e redraws row e with the episode key (the env's autoresets since its explicit reset), which
    the host copy of the draw reproduces; every other row stays."""
    from f110_gymnasium_ros2_jazzy_amd.sim import param_range_rows
    E, A, T = 16, 1, 130
    spawn = np.array([[[10.0 + 5 * i, y, np.pi / 2]] for i, y in enumerate((0.6, 0.8, 0.9, 1.0))])
    ranges = {"mu": (0.6, 1.1), "a_max": (6.0, 11.0), "m": M}
    lo, hi = param_range_rows(ranges, [_defaults()])
    sims = [_sim(tracks, gpu, "straight_corridor", n_envs=E, n_agents=A, autoreset=True, spawn_poses=spawn, seed=21)
            for _ in range(2)]
    poses = spawn[np.arange(E) % 4]
    for s in sims:
        s.set_param_randomization(ranges, seed=77)
        s.reset(poses)
    crash = np.tile([[[0.0, 20.0]]], (E, 1, 1)).astype(np.float32)
    prev = _table(sims[0])
    for e in range(E):
        assert np.array_equal(prev[e, 0, :16], _host_draw(77, e, 0, 0, lo[0], hi[0])[:16])
    episodes = np.zeros(E, int)
    for t in range(T):
        was = sims[0].step(crash).was_reset.cpu().numpy().astype(bool)
        sims[1].step(crash)
        cur = _table(sims[0])
        episodes += was
        assert np.array_equal(np.any(cur != prev, axis=(1, 2)), was), t
        for e in np.flatnonzero(was):
            assert np.array_equal(cur[e, 0, :16], _host_draw(77, e, 0, int(episodes[e]), lo[0], hi[0])[:16]), (e, t)
        prev = cur
    assert episodes.min() >= 2  # every env went through its second autoreset at least
    assert np.array_equal(_table(sims[1]), prev)  # an identical context draws the same cars
    assert np.array_equal(sims[1].get_state()[0].cpu().numpy(), sims[0].get_state()[0].cpu().numpy())
    # an explicit reset restarts the episode count
    sims[0].reset(poses)
    t0 = _table(sims[0])
    for e in range(E):
        assert np.array_equal(t0[e, 0, :16], _host_draw(77, e, 0, 0, lo[0], hi[0])[:16])
    for s in sims:
        s.close()


def test_draw_is_in_force_in_the_resets_own_step(tracks, gpu):
    """The row read back after a reset is the car in force from the reset's own zero-action step on:
    a one-env context given that row follows the randomized env bit for bit through the reset and
    the steps after it."""
    E, A, T = 5, 1, 10
    rng = np.random.default_rng(17)
    sp = _spawns(A)
    poses = sp[::900][:E]
    acts = _actions(rng, T, E, A)
    ranges = {"mu": MU, "m": M, "a_max": (6.0, 11.0), "sv_max": (2.0, 4.0), "C_Sf": (3.5, 5.5)}
    sim = _sim(tracks, gpu, n_envs=E, n_agents=A)
    sim.set_param_randomization(ranges, seed=5)
    sim.reset(poses)
    rows = sim.env_params()
    states = [sim.get_state()[0].cpu().numpy()]
    for t in range(T):
        sim.step(acts[t])
        states.append(sim.get_state()[0].cpu().numpy())
    assert all(np.array_equal(v, rows[k]) for k, v in sim.env_params().items())  # no reset since: the rows stay
    for e in range(E):
        one = _sim(tracks, gpu, n_envs=1, n_agents=A, env_offset=e)
        one.set_env_params({k: v[e:e + 1] for k, v in rows.items()})
        one.reset(poses[e:e + 1])
        for t in range(T + 1):
            if t:
                one.step(acts[t - 1, e:e + 1])
            assert np.array_equal(one.get_state()[0].cpu().numpy()[:, 0], states[t][:, e]), (e, t)
        one.close()
    sim.close()


def test_step_n_and_graph_replay(tracks, gpu):
    """25 steps with autoreset and randomization on, as 25 step calls, one step_n call and 25 replays
    of one captured step: the same states and the same table.  The cars face the track's wall at
    full speed and first crash around step 43, inside the compared window."""
    E, A, PRE, N = 64, 1, 30, 25
    sp = _spawns(A)
    poses = sp[::80][:E].copy()
    poses[:, 0, 2] += np.pi / 2
    ranges = {"mu": (0.6, 1.1), "a_max": (6.0, 11.0), "m": M}
    act = torch.tensor([0.0, 20.0], device=gpu).repeat(E, A, 1).contiguous()
    sims = [_sim(tracks, gpu, n_envs=E, n_agents=A, autoreset=True, spawn_poses=sp, seed=13, noise_std=0.01)
            for _ in range(3)]
    for s in sims:
        s.set_param_randomization(ranges, seed=99)
        s.reset(poses)
        for _ in range(PRE):
            s.step(act)
    before = _table(sims[0])
    for _ in range(N):
        sims[0].step(act)
    sims[1].step_n(act.unsqueeze(0).repeat(N, 1, 1, 1))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sims[2].step(act)
    for _ in range(N):
        g.replay()
    torch.cuda.synchronize()
    ref_state, ref_table = sims[0].get_state()[0].cpu().numpy(), _table(sims[0])
    assert np.any(ref_table != before, axis=(1, 2)).sum() >= E // 4  # autoresets did redraw inside the window
    for s in sims[1:]:
        assert np.array_equal(s.get_state()[0].cpu().numpy(), ref_state)
        assert np.array_equal(_table(s), ref_table)
        assert np.array_equal(s.out.obs.cpu().numpy(), sims[0].out.obs.cpu().numpy())
    for s in sims:
        s.close()


def test_vector_env_param_ranges(gpu):
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    with pytest.raises(ValueError, match="nope"):
        F110VectorEnv(8, param_ranges={"nope": (0, 1)}, device=gpu)
    env = F110VectorEnv(64, num_agents=1, param_ranges={"mu": MU, "m": M}, device=gpu)
    try:
        d = _defaults()
        assert (env.sim.env_params()["mu"] == d["mu"]).all()  # applied at resets: the first one is still to come
        obs, infos = env.reset(seed=1)
        p = env.sim.env_params()
        assert len(np.unique(p["mu"])) == 64 and (p["mu"] >= MU[0]).all() and (p["mu"] < MU[1]).all()
        assert (p["m"] >= M[0]).all() and (p["m"] < M[1]).all() and (p["lf"] == d["lf"]).all()
        keys = set(infos)
        out = env.step(torch.zeros(64, 2, device=env.device))
        assert len(out) == 5 and tuple(out[0].shape) == (64, 1084) and out[1].shape == (64,)
        assert set(out[4]) == keys and "params" not in keys
    finally:
        env.close()
