"""Spawn randomization, host side (no GPU): the new entry points are exported, the validation of
f110_set_spawn_randomization refuses what it must (through its host hook: no context can be created
here), the row rule (csrc/f110_spawn.h through f110_host_spawn_rows) draws what the header states,
clears the lateral offset against the EDT, wraps the gap at both table ends, and the Python helpers
and the trainer's flags build the ranges the C ABI takes."""
import argparse
import ctypes

import numpy as np
import pytest

N_DRAWS = 5000  # envs x 2 agents = 10^4 cars


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def corridor(tracks):
    return tracks("straight_corridor")  # along x, free for y in (-0.9, 1.35); off-map lookups read 0


def _rows(ranges, A=2):
    from f110_gymnasium_ros2_jazzy_amd.sim import spawn_range_rows
    return spawn_range_rows(ranges, A)


def _check(F, ranges, A=1, n_spawn=8):
    L = F.load()
    rc = L.f110_host_check_spawn_ranges(_rows(ranges, A), A, n_spawn)
    return rc, (L.f110_last_error() or b"").decode()


def _host(*a, **kw):
    from f110_gymnasium_ros2_jazzy_amd.sim import host_spawn_rows
    return host_spawn_rows(*a, **kw)


def _edt_at(F, track, x, y):
    """The EDT value a lookup at (x, y) reads (f110_host_cell_index over track.dt())."""
    xy = np.ascontiguousarray(np.stack([np.atleast_1d(x), np.atleast_1d(y)], 1), dtype=np.float64)
    lin = np.empty((xy.shape[0], 3), np.int64)
    org = (ctypes.c_double * 3)(*track.origin)
    assert F.load().f110_host_cell_index(track.height, track.width, track.resolution, org, xy.ctypes.data,
                                         xy.shape[0], lin.ctypes.data) == 0
    return np.ascontiguousarray(track.dt()).ravel()[lin[:, 0]]


def test_exports_and_abi(F):
    L = F.load()
    for n in ("f110_set_spawn_randomization", "f110_get_spawn_state", "f110_host_check_spawn_ranges",
              "f110_host_spawn_rows"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == F.ABI_VERSION
    assert ctypes.sizeof(F.F110SpawnRange) == 72 == F.SPAWN_RANGE_BYTES
    assert F.SPAWN_FIELDS == ("lateral", "heading", "speed", "gap", "behind", "clearance")
    assert F.F110SpawnRange.gap.offset == 48 and F.F110SpawnRange.behind.offset == 56


def test_validation_accepts(F):
    assert _check(F, {})[0] == 0  # all zero: the base pose at rest
    full = {"lateral": (-0.3, 0.3), "heading": (-0.2, 0.2), "speed": (1.0, 6.0), "gap": (5, 12), "behind": 0.5,
            "clearance": 0.3}
    assert _check(F, full)[0] == 0
    assert _check(F, [{"lateral": (0.1, 0.1)}, full], A=2)[0] == 0
    assert _check(F, {"behind": 1.0, "speed": (-1.0, 0.0)}, n_spawn=0)[0] == 0  # no gap: no table needed


@pytest.mark.parametrize("field", ["lateral", "heading", "speed"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_validation_refuses_non_finite(F, field, bad):
    for pair in ((bad, 1.0), (0.0, bad)):
        rc, msg = _check(F, {field: pair})
        assert rc == -1 and field in msg.split(":")[1], msg


@pytest.mark.parametrize("field", ["lateral", "heading", "speed", "gap"])
def test_validation_refuses_lo_above_hi(F, field):
    rc, msg = _check(F, {field: (3, 2)})
    assert rc == -1 and field in msg.split(":")[1] and "lo > hi" in msg


def test_validation_refuses_the_rest(F):
    for ranges, field in (({"gap": (-1, 2)}, "gap"), ({"gap": (-3, -2)}, "gap"), ({"behind": -0.01}, "behind"),
                          ({"behind": 1.01}, "behind"), ({"behind": float("nan")}, "behind"),
                          ({"clearance": -0.1}, "clearance"), ({"clearance": float("inf")}, "clearance")):
        rc, msg = _check(F, ranges)
        assert rc == -1 and field in msg.split(":")[1], (ranges, msg)
    rc, msg = _check(F, {"gap": (0, 3)}, n_spawn=0)
    assert rc == -1 and "gap" in msg and "spawn table" in msg
    # the second agent's block is checked, and named
    rc, msg = _check(F, [{}, {"speed": (2.0, 1.0)}], A=2)
    assert rc == -1 and "speed" in msg and "agent 1" in msg
    L = F.load()
    assert L.f110_host_check_spawn_ranges(None, 1, 0) == -1
    assert L.f110_host_check_spawn_ranges(_rows({}, 1), 0, 0) == -1


RANGES = {"lateral": (-0.3, 0.3), "heading": (-0.2, 0.2), "speed": (1.0, 6.0)}


@pytest.fixture(scope="module")
def draws(corridor):
    """10^4 cars' reset draws from base (20, 0, 0): there sin = 0, cos = 1 and the corridor is wide, so
    y is the lateral draw itself, yaw the heading draw and x stays 20."""
    envs = np.arange(N_DRAWS)
    poses = np.tile([20.0, 0.0, 0.0], (N_DRAWS, 2, 1))
    out, rows = _host(RANGES, 7, corridor, envs, 2, poses=poses)
    assert (rows == -1).all()
    return envs, poses, out


def test_draws_lie_in_their_ranges(draws):
    _, _, out = draws
    assert (out[..., 0] == 20.0).all()
    for col, key in ((1, "lateral"), (2, "heading"), (3, "speed")):
        lo, hi = RANGES[key]
        v = out[..., col]
        assert (v >= lo).all() and (v < hi).all(), key
        assert len(np.unique(v)) > 0.99 * v.size
        se = (hi - lo) / np.sqrt(12.0 * v.size)  # the uniform law's standard error of the mean
        assert abs(v.mean() - 0.5 * (lo + hi)) < 5 * se, key
        # lo + u (hi - lo) for a u on the 2^-32 grid, evaluated without a fused multiply-add
        r = np.round((v - lo) / (hi - lo) * 2.0 ** 32)
        assert np.array_equal(v, lo + (r * 2.0 ** -32) * (hi - lo)), key
    assert abs(np.corrcoef(out[..., 1].ravel(), out[..., 2].ravel())[0, 1]) < 0.05
    assert not np.array_equal(out[:, 0], out[:, 1])  # the agents draw their own


def test_degenerate_ranges_are_exact(corridor, draws):
    envs, poses, _ = draws
    out, _ = _host({"lateral": (0.1, 0.1), "heading": (-0.25, -0.25), "speed": (3.5, 3.5)}, 7, corridor, envs[:64], 2,
                   poses=poses[:64])
    assert (out[..., 1] == 0.1).all() and (out[..., 2] == -0.25).all() and (out[..., 3] == 3.5).all()
    out, _ = _host({}, 7, corridor, envs[:64], 2, poses=poses[:64])
    assert np.array_equal(out[..., :3], poses[:64]) and (out[..., 3] == 0.0).all()


def test_draw_is_a_function_of_its_key(corridor, draws):
    envs, poses, out = draws
    e, p = envs[:16], poses[:16]
    base = out[:16]
    again, _ = _host(RANGES, 7, corridor, e, 2, poses=p, ctx_seed=99)  # the context's seed is no part of it
    assert np.array_equal(again, base)
    for kw in (dict(seed=8), dict(seed=7 + (1 << 32)), dict(episodes=np.ones(16, np.uint64)),
               dict(episodes=np.full(16, 1 << 32, np.uint64))):
        other, _ = _host(RANGES, kw.pop("seed", 7), corridor, e, 2, poses=p, **kw)
        assert (other[..., 1:] != base[..., 1:]).all(), kw
    shifted, _ = _host(RANGES, 7, corridor, e + 1, 2, poses=p)
    assert np.array_equal(shifted[:-1], base[1:]) and (shifted[0] != base[0])[:, 1:].all()  # keyed by the env id
    far, _ = _host(RANGES, 7, corridor, e + (1 << 32), 2, poses=p)
    assert (far[..., 1:] != base[..., 1:]).all()
    # the base pose moves the result, not the draw
    moved, _ = _host(RANGES, 7, corridor, e, 2, poses=p + [1.0, 0.0, 0.0])
    assert np.array_equal(moved[..., 1:], base[..., 1:]) and (moved[..., 0] == 21.0).all()


def _table(n):
    sp = np.zeros((n, 2, 3))
    sp[:, :, 0] = 5.0 + 0.05 * np.arange(n)[:, None]
    sp[:, 1, 1] = 0.5  # the second column: another pose of the same row
    return sp


def test_gap_and_behind_frequencies(corridor):
    n, k, lo, hi, p = 1000, 500, 5, 12, 0.3
    sp = _table(n)
    envs = np.arange(2 * N_DRAWS)
    out, rows = _host([{}, {"gap": (lo, hi), "behind": p}], 7, corridor, envs, 2, spawn=sp,
                      rows=np.full(envs.size, k, np.int32), episodes=np.ones(envs.size, np.uint64))
    assert (rows[:, 0] == k).all() and np.array_equal(out[:, 0, :3], np.tile(sp[k, 0], (envs.size, 1)))
    shift = rows[:, 1] - k
    assert set(np.abs(shift)) == set(range(lo, hi + 1))  # the magnitudes cover [lo, hi] inclusive
    assert np.array_equal(out[:, 1, :3], sp[rows[:, 1], 0])  # column 0 of the shifted row
    freq, sigma = (shift < 0).mean(), np.sqrt(p * (1 - p) / envs.size)
    print(f"behind frequency {freq:.4f}, expected {p} +- {sigma:.4f}")
    assert abs(freq - p) < 4 * sigma
    counts = np.bincount(np.abs(shift))[lo:]
    assert abs(counts - envs.size / (hi - lo + 1)).max() < 5 * np.sqrt(envs.size / (hi - lo + 1))
    # behind 0 / 1: never / always
    for pb, sign in ((0.0, 1), (1.0, -1)):
        _, r = _host([{}, {"gap": (lo, hi), "behind": pb}], 7, corridor, envs[:256], 2, spawn=sp,
                     rows=np.full(256, k, np.int32), episodes=np.ones(256, np.uint64))
        assert (np.sign(r[:, 1] - k) == sign).all()


def test_gap_wraps_at_both_table_ends(corridor):
    n = 50
    sp = _table(n)
    envs = np.arange(n)
    k = np.arange(n, dtype=np.int32)
    ep = np.ones(n, np.uint64)
    for mag in (5, 49, 50, 123):
        _, ahead = _host([{}, {"gap": (mag, mag)}], 3, corridor, envs, 2, spawn=sp, rows=k, episodes=ep)
        _, back = _host([{}, {"gap": (mag, mag), "behind": 1.0}], 3, corridor, envs, 2, spawn=sp, rows=k, episodes=ep)
        assert np.array_equal(ahead[:, 1], (k + mag) % n) and np.array_equal(back[:, 1], (k - mag) % n), mag
        assert np.array_equal(ahead[:, 0], k) and np.array_equal(back[:, 0], k)
    # a gap with magnitude 0 drawn: still column 0, of the env's own row
    out, r = _host([{}, {"gap": (0, 1)}], 3, corridor, envs, 2, spawn=sp, rows=k, episodes=ep)
    assert set(r[:, 1] - k) <= {0, 1, 1 - n} and np.array_equal(out[:, 1, :3], sp[r[:, 1], 0])
    # without rows the env's row is the context's draw, the same for both agents, inside the table
    _, r = _host([{}, {}], 3, corridor, envs, 2, spawn=sp, episodes=ep, ctx_seed=11)
    assert np.array_equal(r[:, 0], r[:, 1]) and r.min() >= 0 and r.max() < n and len(set(r[:, 0])) > n // 3
    from f110_gymnasium_ros2_jazzy_amd._lib import F110Error
    with pytest.raises(F110Error, match="episode"):
        _host([{}, {}], 3, corridor, envs, 2, spawn=sp)  # an autoreset's key is >= 1
    with pytest.raises(F110Error, match="row"):
        _host([{}, {}], 3, corridor, envs, 2, spawn=sp, rows=k + 1, episodes=ep)


@pytest.mark.parametrize("yaw", [0.0, 0.4, np.pi])
def test_clearance_fallback(F, corridor, yaw):
    """A base pose beside the wall (0.45 m at yaw 0): the accepted offset is the first of d, d/2, d/4,
    d/8, 0 whose position reads an EDT value >= clearance, and exactly that value."""
    c, n = 0.3, 400
    px, py = 20.0, 0.9
    sn, cs = np.empty(1), np.empty(1)
    F.load().f110_host_sincos(np.array([yaw]).ctypes.data, 1, sn.ctypes.data, cs.ctypes.data)
    envs = np.arange(n)
    poses = np.tile([px, py, yaw], (n, 1, 1))
    free, _ = _host({"lateral": (-2.0, 2.5)}, 5, corridor, envs, 1, poses=poses)  # the raw draws d
    out, _ = _host({"lateral": (-2.0, 2.5), "clearance": c}, 5, corridor, envs, 1, poses=poses)
    # the raw draws from their own definition (the same key, base (0, 0, 0): y is d itself)
    d = _host({"lateral": (-2.0, 2.5)}, 5, corridor, envs, 1, poses=np.zeros((n, 1, 3)))[0][:, 0, 1]
    assert np.array_equal(free[:, 0, 0], px + d * -sn[0]) and np.array_equal(free[:, 0, 1], py + d * cs[0])
    tries = np.stack([d, d * 0.5, d * 0.25, d * 0.125, np.zeros(n)])               # [5, n]
    x, y = px + tries * -sn[0], py + tries * cs[0]
    edt = np.stack([_edt_at(F, corridor, x[i], y[i]) for i in range(5)])
    ok = edt >= c
    ok[4] = True  # d = 0 is always accepted
    first = ok.argmax(0)
    e = np.arange(n)
    assert np.array_equal(out[:, 0, 0], x[first, e]) and np.array_equal(out[:, 0, 1], y[first, e])
    got = _edt_at(F, corridor, out[:, 0, 0], out[:, 0, 1])
    assert (got[first < 4] >= c).all()  # the accepted position meets the clearance whenever d != 0
    assert (out[:, 0, 2] == yaw).all() and (out[:, 0, 3] == 0.0).all()  # heading and speed are never adjusted
    taken = np.bincount(first, minlength=5)
    print("accepted try (d, d/2, d/4, d/8, 0):", taken)
    assert (taken > 0).all()  # every branch of the fallback occurred


def test_out_of_map_lookup_and_f32(F, corridor):
    envs = np.arange(64)
    # a base pose outside the map: every lookup reads the last cell (0 here), so any clearance > 0 drops the offset
    poses = np.tile([500.0, 40.0, 0.3], (64, 1, 1))
    out, _ = _host({"lateral": (0.5, 1.0), "clearance": 0.01, "speed": (1.0, 2.0)}, 1, corridor, envs, 1, poses=poses)
    assert np.array_equal(out[..., :3], poses) and (out[..., 3] >= 1.0).all()
    out0, _ = _host({"lateral": (0.5, 1.0), "speed": (1.0, 2.0)}, 1, corridor, envs, 1, poses=poses)  # clearance 0: kept
    assert (out0[..., 1] != 40.0).all()
    # float32 resets: the pose rounded after the perturbation, the speed not
    poses = np.tile([20.0, 0.1, 0.2], (64, 1, 1))
    r = dict(RANGES, clearance=0.2)
    f64, _ = _host(r, 1, corridor, envs, 1, poses=poses)
    f32, _ = _host(r, 1, corridor, envs, 1, poses=poses, reset_f32=True)
    assert np.array_equal(f32[..., :3], f64[..., :3].astype(np.float32).astype(np.float64))
    assert np.array_equal(f32[..., 3], f64[..., 3]) and not np.array_equal(f32[..., :3], f64[..., :3])


def test_python_rows(F):
    from f110_gymnasium_ros2_jazzy_amd.sim import spawn_range_rows
    rows = spawn_range_rows({"lateral": (-0.3, 0.3), "gap": (5, 12), "behind": 0.5, "clearance": 0.25}, 2)
    assert len(rows) == 2 and ctypes.sizeof(rows) == 144
    for r in rows:
        assert tuple(r.lateral) == (-0.3, 0.3) and tuple(r.heading) == (0.0, 0.0) and tuple(r.speed) == (0.0, 0.0)
        assert tuple(r.gap) == (5, 12) and r.behind == 0.5 and r.clearance == 0.25
    rows = spawn_range_rows([{"speed": (1, 6)}, {"heading": (-0.1, 0.1), "gap": (3, 3)}], 2)
    assert tuple(rows[0].speed) == (1.0, 6.0) and tuple(rows[0].gap) == (0, 0) and tuple(rows[1].speed) == (0.0, 0.0)
    assert tuple(rows[1].heading) == (-0.1, 0.1) and tuple(rows[1].gap) == (3, 3)
    with pytest.raises(ValueError, match="nope"):
        spawn_range_rows({"nope": (0, 1)}, 2)
    with pytest.raises(ValueError, match="per agent"):
        spawn_range_rows([{"speed": (1, 6)}], 2)
    with pytest.raises(ValueError, match="pair"):
        spawn_range_rows({"speed": 3.0}, 1)
    with pytest.raises(ValueError, match="whole"):
        spawn_range_rows({"gap": (0.5, 2)}, 1)
    assert F.load().f110_host_check_spawn_ranges(rows, 2, 10) == 0  # the library accepts what the helper builds


def test_vector_env_refuses_unknown_key_before_building():
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    with pytest.raises(ValueError, match="nope"):
        F110VectorEnv(4, map="straight_corridor", spawn_ranges={"nope": (0, 1)}, device="cpu")
    with pytest.raises(ValueError, match="per agent"):
        F110VectorEnv(4, map="straight_corridor", num_agents=2, spawn_ranges=[{}], device="cpu")


def test_train_flags():
    from f110_gymnasium_ros2_jazzy_amd.train import add_spawn_args, spawn_ranges_from_args
    ap = argparse.ArgumentParser()
    add_spawn_args(ap)
    assert spawn_ranges_from_args(ap.parse_args([])) is None  # no flag: no call
    args = ap.parse_args(["--spawn-lateral=-0.3,0.3", "--spawn-heading=-0.2,0.2", "--spawn-speed", "1,6",
                          "--spawn-gap", "30,60", "--spawn-behind", "0.5", "--spawn-clearance", "0.4"])
    every = {"lateral": (-0.3, 0.3), "heading": (-0.2, 0.2), "speed": (1.0, 6.0), "clearance": 0.4}
    assert spawn_ranges_from_args(args) == [every, dict(every, gap=(30, 60), behind=0.5)]  # gap, behind: the opponent
    assert spawn_ranges_from_args(ap.parse_args(["--spawn-speed", "2,3"])) == [{"speed": (2.0, 3.0)}] * 2
    assert spawn_ranges_from_args(ap.parse_args(["--spawn-gap", "10,20"])) == [{}, {"gap": (10, 20)}]
    for bad in (["--spawn-speed", "2"], ["--spawn-gap", "1.5,2"], ["--spawn-lateral", "a,b"]):
        with pytest.raises(ValueError, match=bad[0]):
            spawn_ranges_from_args(ap.parse_args(bad))
    from f110_gymnasium_ros2_jazzy_amd.sim import spawn_range_rows
    spawn_range_rows(spawn_ranges_from_args(args), 2)  # and the env takes them
