"""The pure-pursuit opponent, host side (no GPU): f110_host_pure_pursuit -- the statement of
f110_pure_pursuit over host arrays -- against a NumPy restatement of the controller (projection:
oracle/reward_oracle.py's TrackOracle) on the Spielberg centerline and three small tracks, its
argument errors, the argument validation of F110VectorEnv and VectorTrainer, and a closed loop on
the CPU oracle simulator: both cars of 8 envs lap Spielberg on the statement's actions.

The closed loop as recorded with the library's defaults (lookahead 1.2 m, 4.0 m/s, 1500 steps, 16
cars): no collision, progress 60.57 .. 63.07 m (nominal 60 m), max |t| 0.280 m (lane half
width 0.97 m)."""
import ctypes
import os

import numpy as np
import pytest

import pursuit_cases as C
from conftest import MAPS


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def O():
    from f110_gymnasium_ros2_jazzy_amd import opponent
    return opponent


@pytest.fixture(scope="module")
def cases():
    """name -> (host-only CenterlineTrack, TrackOracle, poses float32 [M, 3]); built once."""
    import reward_oracle as R
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    out = {}
    xy, wr, wl = C.spielberg_xy()
    named = {"spielberg": (xy, True), **C.small_tracks()}
    for name, (pts, closed) in named.items():
        T = R.TrackOracle(pts, closed=closed)
        tr = CenterlineTrack(pts, closed=closed, device=None)
        poses = np.concatenate([C.track_poses(T, spread=3.0 if name == "spielberg" else 1.5), C.special_poses()])
        out[name] = (tr, T, poses)
    yield out
    for tr, _, _ in out.values():
        tr.close()


def test_exports(F):
    L = F.load()
    for n in ("f110_default_pursuit_params", "f110_pure_pursuit", "f110_host_pure_pursuit"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION
    p = F.F110PursuitParams()
    L.f110_default_pursuit_params(ctypes.byref(p))
    car = F.default_params()
    assert {k: getattr(p, k) for k in C.DEFAULTS} == {**C.DEFAULTS, "wheelbase": car.lf + car.lr}
    assert abs(p.wheelbase - 0.3302) < 1e-15
    assert ctypes.sizeof(p) == 56


@pytest.mark.parametrize("name", ["spielberg", "open4", "triangle", "repeated", "cluster"])
def test_matches_restatement(F, O, cases, name):
    tr, T, poses = cases[name]
    L = F.load()
    la = 1.2 if name == "spielberg" else 1.0
    assert np.array_equal(tr.s, T.s) and tr.L == T.L  # the library's track is the oracle's
    for kw in (dict(lookahead=la), dict(lookahead=la, direction=-1), dict(lookahead=la, speed=2.5, steer_limit=0.05),
               dict(lookahead=la, a_lat=6.0, speed=12.0), dict(lookahead=la, a_lat=0.5, v_floor=1.5, speed=8.0)):
        want_a, want_x = C.np_pursuit(L, T, poses, **kw)
        got_a, got_x = O.host_pure_pursuit(poses, tr, return_aux=True, **kw)
        C.assert_aux_equal(got_x, want_x, (name, kw))
        C.assert_actions_close(got_a, want_a, (name, kw))
        finite = np.isfinite(poses).all(axis=1)
        assert (got_a[~finite] == 0.0).all() and not finite.all()
        if not kw.get("a_lat"):  # constant speed: exact, whatever the steering does
            assert (got_a[finite, 1] == np.float32(kw.get("speed", 4.0))).all()
        if "steer_limit" in kw:  # the clip is active on some rows, and exact there
            lim = np.float32(kw["steer_limit"])
            assert (np.abs(got_a[finite, 0]) <= lim).all() and (np.abs(got_a[finite, 0]) == lim).sum() >= 3
        if kw.get("a_lat") == 0.5:  # the profile slows some rows down to the floor and leaves others at the cap
            assert (got_a[finite, 1] == np.float32(1.5)).any() and (got_a[finite, 1] > np.float32(1.5)).any()


def test_pose_on_its_own_target(F, O, cases):
    """An open track's last node is its own target (the clamp): d2 = 0, steer 0, speed as computed."""
    tr, T, _ = cases["open4"]
    poses = np.array([[12.0, 2.0, 0.7], [12.0, 2.0, -2.0]], np.float32)
    for kw in (dict(lookahead=1.0), dict(lookahead=1.0, a_lat=4.0, speed=30.0)):
        act, aux = O.host_pure_pursuit(poses, tr, return_aux=True, **kw)
        want_a, want_x = C.np_pursuit(F.load(), T, poses, **kw)
        assert np.array_equal(aux[:, 2:], poses[:, :2].astype(np.float64)) and (aux[:, 0] == T.L).all()
        assert (act[:, 0] == 0.0).all() and not np.signbit(act[:, 0]).any()
        C.assert_aux_equal(aux, want_x)
        C.assert_actions_close(act, want_a)
    assert act[0, 1] == np.float32(30.0)  # |kappa| is NaN there: it counts as 1e-9, the cap holds


@pytest.mark.parametrize("M", C.ROWS)
def test_rows_strides_mask_speed(F, O, cases, M):
    tr, T, pool = cases["spielberg"]
    rng = np.random.default_rng(M)
    poses = pool[rng.integers(0, len(pool), M)]
    want_a, want_x = C.np_pursuit(F.load(), T, poses)
    # strided rows: poses inside a wider "obs" row, actions inside an [M, A, 2] buffer
    obs = np.full((M, 11), np.float32(7.0))
    obs[:, 4:7] = poses
    buf = np.full((M, 3, 2), np.float32(np.nan))
    got = O.host_pure_pursuit(obs[:, 4:8], tr, out=buf[:, 1])
    assert got.base is buf or got is buf[:, 1] or np.shares_memory(got, buf)
    C.assert_actions_close(buf[:, 1], want_a, M)
    assert np.isnan(buf[:, 0]).all() and np.isnan(buf[:, 2]).all()  # the neighbours' slots are untouched
    # per-row speeds
    speeds = rng.uniform(0.0, 9.0, M)
    want_s, _ = C.np_pursuit(F.load(), T, poses, row_speed=speeds)
    got_s, aux = O.host_pure_pursuit(poses, tr, row_speed=speeds, return_aux=True)
    C.assert_actions_close(got_s, want_s, M)
    C.assert_aux_equal(aux, want_x, M)
    fin = np.isfinite(poses).all(axis=1)
    assert np.array_equal(got_s[fin, 1], speeds[fin].astype(np.float32))
    # masked rows keep their bytes (poisoned with NaN patterns first)
    mask = (rng.random(M) < 0.5).astype(np.uint8)
    poison_a = np.full((M, 2), np.float32(np.nan))
    L = F.load()
    p = C.c_params(F)
    poison_x = np.full((M, 4), np.nan)
    assert L.f110_host_pure_pursuit(tr.handle, ctypes.byref(p), poses.ctypes.data, M, 3, None, mask.ctypes.data,
                                    poison_a.ctypes.data, 2, poison_x.ctypes.data) == 0
    keep = mask == 0
    assert np.isnan(poison_a[keep]).all() and np.isnan(poison_x[keep]).all()
    C.assert_actions_close(poison_a[~keep], want_a[~keep], M)
    C.assert_aux_equal(poison_x[~keep], want_x[~keep], M)


def test_error_paths(F, cases):
    L = F.load()
    tr = cases["spielberg"][0]
    M = 4
    poses = np.zeros((M, 3), np.float32)
    act = np.zeros((M, 2), np.float32)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(fn=L.f110_host_pure_pursuit, track=tr.handle, poses_p=P(poses), n=M, ps=3, act_p=P(act), as_=2, extra=(),
             null_params=False, **params):
        p = C.c_params(F, **params)
        return fn(track, None if null_params else ctypes.byref(p), poses_p, n, ps, None, None, act_p, as_, None, *extra)

    assert call() == 0
    bad = [dict(track=None), dict(poses_p=None), dict(act_p=None), dict(null_params=True), dict(ps=2), dict(as_=1),
           dict(n=-1), dict(lookahead=0.0), dict(lookahead=-1.0), dict(lookahead=tr.L), dict(lookahead=1e9),
           dict(lookahead=float("nan")), dict(wheelbase=0.0), dict(wheelbase=-0.3), dict(steer_limit=0.0),
           dict(steer_limit=-0.4), dict(speed=-0.1), dict(speed=float("nan")), dict(a_lat=-1.0), dict(direction=0),
           dict(direction=2)]
    for kw in bad:
        assert call(**kw) == -1, kw  # F110_E_INVALID
        assert b"f110_host_pure_pursuit" in L.f110_last_error()
        # the device entry refuses the same arguments before any device call
        assert call(fn=L.f110_pure_pursuit, extra=(C.NULL,), **kw) == -1, kw
        assert b"f110_pure_pursuit" in L.f110_last_error()
    # a host-only track (device < 0) at the device entry
    assert call(fn=L.f110_pure_pursuit, extra=(C.NULL,)) == -1
    assert b"device track" in L.f110_last_error()
    assert call(speed=0.0, n=0) == 0  # the edges that are allowed


def test_python_argument_checks(O, cases):
    tr = cases["open4"][0]
    poses = np.zeros((3, 3), np.float32)
    for kw in (dict(poses=poses.astype(np.float64)), dict(poses=poses[:, :2]), dict(poses=poses[0]),
               dict(out=np.zeros((3, 3), np.float32)), dict(out=np.zeros((3, 2), np.float64)),
               dict(row_speed=np.zeros(4)), dict(row_mask=np.zeros(2, np.uint8)), dict(gain=1.0), dict(direction=0),
               dict(track=None)):
        args = dict(poses=poses, track=tr, lookahead=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            O.host_pure_pursuit(args.pop("poses"), args.pop("track"), **args)
    from f110_gymnasium_ros2_jazzy_amd import _lib
    with pytest.raises(_lib.F110Error, match="f110_host_pure_pursuit"):
        O.host_pure_pursuit(poses, tr, lookahead=100.0)  # >= L: the library's check


class _FakeTrack:  # what F110VectorEnv checks of a CenterlineTrack on the host
    def __init__(self, device):
        import torch
        self.device, self.handle = (None if device is None else torch.device(device)), 1


class _FakePolicy:
    def __init__(self, n_envs, act_dim=2, lidar_max=30.0):
        self.n_envs, self.act_dim, self.lidar_max = n_envs, act_dim, lidar_max


def test_vector_env_argument_validation():
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    kw = dict(num_agents=2, device="cpu")  # nothing may be built: a build on this device would fail otherwise
    ok = _FakeTrack("cpu")
    with pytest.raises(ValueError, match="'pure_pursuit'"):
        F110VectorEnv(4, opponent="nonsense", **kw)
    with pytest.raises(ValueError, match="opponent_track"):
        F110VectorEnv(4, opponent="pure_pursuit", **kw)
    with pytest.raises(ValueError, match="opponent_track"):  # a host-only track
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=_FakeTrack(None), **kw)
    with pytest.raises(ValueError, match="opponent_track is on"):  # a foreign device
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=_FakeTrack("cuda:1"), num_agents=2, device="cuda:0")
    with pytest.raises(ValueError, match="opponent_track is on"):
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=_FakeTrack("cuda:0"), **kw)
    with pytest.raises(ValueError, match="opponent_speed"):
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=ok, opponent_speed=np.ones(5), **kw)
    with pytest.raises(ValueError, match="opponent_speed"):
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=ok, opponent_speed=-1.0, **kw)
    with pytest.raises(ValueError, match="opponent_params"):
        F110VectorEnv(4, opponent="pure_pursuit", opponent_track=ok, opponent_params={"gain": 1.0}, **kw)
    with pytest.raises(ValueError, match="num_agents >= 2"):
        F110VectorEnv(4, num_agents=1, device="cpu", opponent="pure_pursuit", opponent_track=ok)
    mixed = dict(opponent="mixed", opponent_policy=_FakePolicy(4), opponent_mask=np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match="opponent_rule"):
        F110VectorEnv(4, opponent_rule="nonsense", **mixed, **kw)
    with pytest.raises(ValueError, match="opponent_track"):
        F110VectorEnv(4, opponent_rule="pure_pursuit", **mixed, **kw)
    with pytest.raises(ValueError, match="opponent_policy"):  # the policy's checks still come
        F110VectorEnv(4, opponent="mixed", opponent_rule="pure_pursuit", opponent_track=ok,
                      opponent_mask=np.zeros(4, np.uint8), **kw)


def test_trainer_argument_validation():
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    for kw in (dict(opponent="pursuit"), dict(opponent="pure_pursuit", opponent_speed=-1.0),
               dict(opponent="pure_pursuit", opponent_speed=np.ones(5)),
               dict(opponent="pure_pursuit", opponent_speed=float("nan")),
               dict(opponent="pure_pursuit", opponent_lookahead=0.0),
               dict(opponent="pure_pursuit", opponent_lookahead=float("nan")),
               dict(opponent="self", selfplay_fraction=0.5, opponent_rule="nonsense")):
        with pytest.raises(ValueError, match="opponent"):
            VectorTrainer(4, device="cpu", **kw)


def test_closed_loop_on_the_cpu_simulator(F, O, cases, oracle_mod):
    """8 envs of 2 cars on Spielberg (default vehicle parameters), spawned on the centerline at
    evenly spaced points, the ego 200 points ahead of the opponent; both cars take
    host_pure_pursuit's actions (library defaults) from their float32 poses for 1500 steps."""
    tr, T, _ = cases["spielberg"]
    free, res, org = oracle_mod.load_map(os.path.join(MAPS, "Spielberg_map.yaml"))
    sim = oracle_mod.OracleSim(oracle_mod.OracleScanner(free, res, org), 8, 2)
    sim.reset(C.lap_spawns(T))
    prog = C.Progress(T, 16)
    collided = False
    for _ in range(1500):
        poses = np.ascontiguousarray(sim.state[:, [0, 1, 4]], dtype=np.float32)
        act, aux = O.host_pure_pursuit(poses, tr, return_aux=True)
        prog.update(aux)
        _, cols = sim.step(act.astype(np.float64), threads=8)
        collided = collided or bool(cols.any())
    print(f"progress {prog.total.min():.3f} .. {prog.total.max():.3f} m, max |t| {prog.max_t:.4f} m, "
          f"collided {collided}")
    assert not collided
    assert (prog.total >= 0.9 * 60.0).all()
    assert prog.max_t <= 0.5
