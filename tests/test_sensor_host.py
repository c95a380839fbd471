"""The sensor randomization, host side (no GPU): f110_host_sensor_apply -- the statement of
f110_sensor_apply over host arrays -- against a NumPy restatement of the row rule
(tests/sensor_cases.py), bit for bit; the identity; sharding independence; the counters and the
mask; the extreme parameters; the statistics of the draws against bounds derived from the model;
and every argument error."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import sensor_cases as C


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def S():
    from f110_gymnasium_ros2_jazzy_amd import sensor
    return sensor


def assert_state(lib, ref, what):
    for k in ("params", "episode", "step"):
        assert C.same_bits(lib[k], ref[k]), (what, k)


def test_exports_and_defaults(F, S):
    L = F.load()
    for n in ("f110_default_sensor_params", "f110_sensor_create", "f110_sensor_destroy", "f110_sensor_apply",
              "f110_sensor_reset", "f110_sensor_arrays", "f110_host_sensor_apply", "f110_host_check_sensor_params"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3
    p = S.sensor_ranges()
    assert ctypes.sizeof(p) == 64 and S.SENSOR_FIELDS == C.NAMES
    for n in C.NAMES:
        assert tuple(getattr(p, n)) == C.IDENTITY[n]
    q = S.sensor_ranges(1080, noise_abs=(0.005, 0.03), dropout=0.25, blackout=(0, 1080))
    assert tuple(q.noise_abs) == (np.float32(0.005), np.float32(0.03)) and tuple(q.dropout) == (0.25, 0.25)
    assert tuple(q.blackout) == (0.0, 1080.0) and tuple(q.scale) == (1.0, 1.0)
    st = S.host_sensor_state(3)
    assert st["params"].shape == (3, 10) and len(S.PARAM_ROW) == 10 and (st["episode"] == -1).all()


@pytest.mark.parametrize("B", C.BEAMS)
def test_matches_restatement(S, B):
    """Six applies with every parameter active, a reset flag for one env at the third; strided rows
    into a strided out and, for the other middle width, in place."""
    for M, T in itertools.product(C.MIDS, C.TAILS):
        for in_place in (False, True):
            rng = np.random.default_rng(B * 10 + M)
            kw = dict(range_max=C.RANGE_MAX, seed=C.SEED, env_offset=C.ENV_OFFSET)
            lib, ref = S.host_sensor_state(C.N_ENVS), C.fresh(C.N_ENVS)
            W = B + M + T
            for t in range(C.APPLIES):
                rows = C.rows_for(rng, C.N_ENVS, B, M, T, stride=W + 3)
                reset = None
                if t == C.RESET_AT:
                    reset = np.zeros(C.N_ENVS, np.uint8)
                    reset[C.RESET_ENV] = 1
                want = C.apply(ref, rows, B, M, T, C.active(B), reset=reset, **kw)
                out = rows if in_place else np.full((C.N_ENVS, W + 2), np.float32(-7.0))[:, :W]
                got = S.host_sensor_apply(lib, rows, B, M, T, reset=reset, out=out, **kw, **C.active(B))
                assert got is out and C.same_bits(got, want), (M, T, in_place, t)
                assert (out.base[:, W:] == np.float32(-7.0)).all()  # the neighbours of strided rows are kept
                assert_state(lib, ref, (M, T, in_place, t))
            assert lib["episode"].tolist() == [0, 1, 0] and lib["step"].tolist() == [5, 3, 5]
            if B > 1:
                assert not C.same_bits(got[:, :B], rows[:, :B]) or in_place


def test_identity_returns_the_row(S):
    rng = np.random.default_rng(3)
    B, M, T = 1080, 8, 5
    rows = C.rows_for(rng, 3, B, M, T)
    rows[0, :6] = [0.0, 1.0, np.float32(1e-42), np.float32(1.4e-45), -0.0, np.float32(1.17549435e-38)]
    rows[1, B + 2] = np.float32(-0.0)
    st = S.host_sensor_state(3)
    for t in range(3):
        reset = np.array([0, 1, 0], np.uint8) if t == 1 else None
        assert C.same_bits(S.host_sensor_apply(st, rows, B, M, T, reset=reset, seed=5), rows)
    assert st["episode"].tolist() == [0, 1, 0]
    row = st["params"][0].tolist()
    assert row == [1.0, 0.0, 0.0, 0.0, 0.0, row[5], 0.0, 0.0, 0.0, 0.0] and 0 <= row[5] <= B


def test_sharding_independence(S):
    """Env 5 of eight (env_offset 0) and the only env of a shard that begins at 5: the same bits."""
    rng = np.random.default_rng(4)
    B, M, T = 130, 8, 5
    whole, part = S.host_sensor_state(8), S.host_sensor_state(1)
    for t in range(4):
        rows = C.rows_for(rng, 8, B, M, T)
        reset = (np.arange(8) == 5).astype(np.uint8) if t == 2 else None
        a = S.host_sensor_apply(whole, rows, B, M, T, seed=C.SEED, env_offset=0, reset=reset, **C.active(B))
        b = S.host_sensor_apply(part, rows[5:6], B, M, T, seed=C.SEED, env_offset=5,
                                reset=None if reset is None else reset[5:6], **C.active(B))
        assert C.same_bits(a[5:6], b), t
        assert C.same_bits(whole["params"][5:6], part["params"]) and not C.same_bits(a[4:5], b)
    assert not C.same_bits(whole["params"][4], whole["params"][5])


def test_reset_redraws_and_mask_passes_through(S):
    rng = np.random.default_rng(6)
    B, M, T = 65, 4, 0
    mask = np.array([1, 0, 1, 0], np.uint8)
    st, free = S.host_sensor_state(4), S.host_sensor_state(4)
    kw = dict(seed=9, **C.active(B))
    before = None
    for t in range(5):
        rows = C.rows_for(rng, 4, B, M, T)
        reset = np.array([0, 0, 1, 1], np.uint8) if t == 3 else None
        out = S.host_sensor_apply(st, rows, B, M, T, mask=mask, reset=reset, **kw)
        ref = S.host_sensor_apply(free, rows, B, M, T, reset=reset, **kw)
        assert C.same_bits(out[1], rows[1]) and C.same_bits(out[3], rows[3])  # masked off: the clean rows
        assert C.same_bits(out[0], ref[0]) and C.same_bits(out[2], ref[2]) and not C.same_bits(out[0], rows[0])
        assert_state(st, free, t)  # the counters and rows advance whatever the mask says
        if t == 2:
            before = st["params"].copy()
    assert st["episode"].tolist() == [0, 0, 1, 1] and st["step"].tolist() == [4, 4, 1, 1]
    assert C.same_bits(st["params"][:2], before[:2])
    assert not C.same_bits(st["params"][2], before[2]) and not C.same_bits(st["params"][3], before[3])


def test_extreme_parameters(S):
    rng = np.random.default_rng(8)
    B, M, T = 130, 4, 5
    rows = C.rows_for(rng, 3, B, M, T)
    one = lambda **r: S.host_sensor_apply(S.host_sensor_state(3), rows, B, M, T, seed=2, **r)  # noqa: E731
    out = one(dropout=1.0)
    assert (out[:, :B] == 1.0).all() and C.same_bits(out[:, B:], rows[:, B:])
    out = one(blackout=B, dropout=1.0, noise_abs=0.5)
    assert (out[:, :B] == 0.0).all()
    assert C.same_bits(one(blackout=0), rows)
    st = S.host_sensor_state(3)
    out = S.host_sensor_apply(st, rows, B, M, T, seed=2, blackout=(10, 20))
    for e in range(3):
        w, s = int(st["params"][e, 4]), int(st["params"][e, 5])
        assert 10 <= w <= 20 and 0 <= s <= B - w and (out[e, s:s + w] == 0).all()
        keep = np.r_[0:s, s + w:B]
        assert C.same_bits(out[e, keep], rows[e, keep])
    st = S.host_sensor_state(3)
    out = S.host_sensor_apply(st, rows, B, M, T, seed=2, quant=(0.3, 1.5), noise_abs=0.3, scale=(0.9, 1.2))
    for e in range(3):
        q = st["params"][e, 6]
        assert np.float32(0.3) / np.float32(30.0) <= q <= np.float32(1.5) / np.float32(30.0)
        inside = (out[e, :B] > 0) & (out[e, :B] < 1)  # up to the final clamp
        k = np.rint(out[e, :B][inside] / q)
        assert inside.sum() > B // 2 and C.same_bits(out[e, :B][inside], (q * k).astype(np.float32))


# ---- the statistics of the draws: every bound is five standard errors of the model ---------------
STAT_B, STAT_STEPS = 1080, 100


def _stat_run(S, **ranges):
    rows = np.full((1, STAT_B), np.float32(0.5))
    st = S.host_sensor_state(1)
    return np.stack([S.host_sensor_apply(st, rows, STAT_B, 0, 0, seed=77, env_offset=3, **ranges)[0].copy()
                     for _ in range(STAT_STEPS)])


def test_dropout_rate(S):
    p = 0.1
    out = _stat_run(S, dropout=p)
    assert set(np.unique(out)) == {np.float32(0.5), np.float32(1.0)}
    n = out.size
    rate = float((out == 1.0).mean())
    print("dropout rate", rate, "bound", 5 * math.sqrt(p * (1 - p) / n))
    assert abs(rate - p) <= 5 * math.sqrt(p * (1 - p) / n)


def test_noise_moments_and_independence(S):
    sigma_m = 0.3  # metres: 0.01 of the range, so 0.5 +- 5.98 sigma stays far inside (0, 1)
    out = _stat_run(S, noise_abs=sigma_m)
    sigma = float(np.float32(sigma_m) / np.float32(30.0))
    x = (out.astype(np.float64) - 0.5) / sigma  # in units of sigma
    n = x.size
    model_std = math.sqrt(65535.0) / 256.0
    std, mean = float(x.std()), float(x.mean())
    print("std", std, "model", model_std, "bound", 5 / math.sqrt(2 * n), "mean", mean, "bound", 5 / math.sqrt(n))
    assert abs(std - model_std) <= 5 / math.sqrt(2 * n)
    assert abs(mean) <= 5 / math.sqrt(n)
    assert np.abs(x).max() <= 1530 / 256 + 1e-3

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1]), a.size
    for what, (r, m) in (("beams", corr(x[:, :-1], x[:, 1:])), ("steps", corr(x[:-1], x[1:]))):
        print("lag-1 correlation across", what, r, "bound", 5 / math.sqrt(m))
        assert abs(r) <= 5 / math.sqrt(m), what


# ---- refusals ----------------------------------------------------------------------------------
def test_c_entry_refusals(F, S):
    L = F.load()
    B, M, T = 64, 4, 2
    rows = np.zeros((3, B + M + T), np.float32)
    out = np.zeros_like(rows)
    par, ep, st = np.zeros((3, 10), np.float32), np.full(3, -1, np.int32), np.zeros(3, np.int32)
    ok = S.sensor_ranges(B)

    def call(params=ok, n=3, B=B, M=M, T=T, rm=30.0, off=0, r=rows, rs=B + M + T, pr=par, e=ep, s=st, o=out,
             os_=B + M + T):
        a = [None if x is None else x.ctypes.data for x in (r, pr, e, s)]
        o = None if o is None else (o if isinstance(o, int) else o.ctypes.data)
        return L.f110_host_sensor_apply(None if params is None else ctypes.byref(params), n, B, M, T, rm, 1, off, None,
                                        a[0], rs, None, a[1], a[2], a[3], o, os_)
    assert call() == 0
    big = np.zeros((3, 200), np.float32)
    for kw in (dict(params=None), dict(n=0), dict(B=0), dict(B=4097), dict(M=5), dict(M=-4), dict(T=-1), dict(rm=0.0),
               dict(rm=-1.0), dict(rm=float("nan")), dict(off=-1), dict(r=None), dict(pr=None), dict(e=None),
               dict(s=None), dict(o=None), dict(rs=B + M + T - 1), dict(os_=B + M + T - 1),
               dict(o=rows.ctypes.data + 4),                       # one float into rows: a partial overlap
               dict(r=big, rs=200, o=big, os_=100)):               # the same pointer, another stride
        assert call(**kw) == -1, kw
        assert b"f110_host_sensor_apply" in L.f110_last_error()
    assert call(o=rows) == 0  # rows itself: in place
    ep[1] = -2
    assert call() == -1
    ep[1] = -1

    def ranges(**kw):
        p = F.F110SensorParams()
        L.f110_default_sensor_params(ctypes.byref(p))
        for k, (lo, hi) in kw.items():
            getattr(p, k)[0], getattr(p, k)[1] = lo, hi
        return p
    inf, nan = float("inf"), float("nan")
    for kw in (dict(noise_abs=(0.0, inf)), dict(quant=(nan, 1.0)), dict(scale=(-inf, 1.0)),  # a non-finite bound
               dict(noise_abs=(0.2, 0.1)), dict(scale=(1.1, 0.9)), dict(blackout=(5, 4)),    # lo > hi
               dict(dropout=(-0.1, 0.5)), dict(dropout=(0.0, 1.5)),                          # outside [0, 1]
               dict(blackout=(-1, 3)), dict(blackout=(0, B + 1)), dict(blackout=(0.5, 3)),   # outside [0, B], not whole
               dict(noise_abs=(-0.1, 0.1)), dict(noise_rel=(-0.1, 0.1)), dict(pose_xy=(-1.0, 0.0)),
               dict(pose_theta=(-1.0, 0.0)), dict(quant=(-0.1, 0.1)),                        # negative
               dict(scale=(0.0, 1.0)), dict(scale=(-1.0, 1.0))):                             # scale <= 0
        assert call(params=ranges(**kw)) == -1, kw
        assert L.f110_host_check_sensor_params(ctypes.byref(ranges(**kw)), B) == -1, kw
    assert L.f110_host_check_sensor_params(None, B) == -1 and L.f110_host_check_sensor_params(ctypes.byref(ok), 0) == -1
    assert call(params=ranges(blackout=(0, B), dropout=(0.0, 1.0))) == 0
    # the device entries refuse the same before any device call (no device is needed to be refused)
    h = ctypes.c_void_p()
    create = lambda **kw: L.f110_sensor_create(  # noqa: E731
        kw.get("out", ctypes.byref(h)), 0, kw.get("n", 3), kw.get("B", B), kw.get("M", M), kw.get("T", T),
        kw.get("rm", 30.0), 1, kw.get("off", 0), None, kw.get("params", ctypes.byref(ok)))
    for kw in (dict(out=None), dict(params=None), dict(n=0), dict(B=0), dict(B=4097), dict(M=6), dict(T=-1), dict(rm=0.0),
               dict(off=-1), dict(params=ctypes.byref(ranges(dropout=(0.0, 2.0)))),
               dict(params=ctypes.byref(ranges(scale=(0.0, 1.0))))):
        assert create(**kw) == -1, kw
        assert b"f110_sensor_create" in L.f110_last_error()
    for fn in (lambda: L.f110_sensor_apply(None, None, 0, None, None, 0, None), lambda: L.f110_sensor_reset(None, None, None),
               lambda: L.f110_sensor_arrays(None, None, None, None)):
        assert fn() == -1


def test_python_refusals(S):
    for bad in (dict(noise=0.1), dict(noise_abs=(0.2, 0.1)), dict(noise_abs=(0.0, float("inf"))), dict(noise_abs="a,b"),
                dict(noise_abs=(0.1, 0.2, 0.3)), dict(dropout=1.5), dict(dropout=(-0.1, 0.0)), dict(scale=0.0),
                dict(quant=-1.0), dict(pose_xy=-0.1), dict(pose_theta=(-0.1, 0.1)), dict(noise_rel=-0.5),
                dict(blackout=1081), dict(blackout=(0, 2.5)), dict(scale=True), dict(scale=None)):
        with pytest.raises(ValueError):
            S.sensor_ranges(1080, **bad)
    with pytest.raises(ValueError, match="unknown"):
        S.sensor_ranges(noise=0.1)
    assert S.sensor_ranges(1080, blackout=1080) and S.sensor_ranges(blackout=4096)
    with pytest.raises(ValueError):
        S.sensor_ranges(100, blackout=101)
    rows = np.zeros((3, 72), np.float32)
    st = S.host_sensor_state(3)
    for kw in (dict(rows=rows[:, :71]), dict(rows=rows.astype(np.float64)), dict(n_mid=6), dict(n_beams=0),
               dict(range_max=0.0), dict(env_offset=-1), dict(mask=np.ones(2, np.uint8)), dict(mask=np.ones(3)),
               dict(reset=np.zeros(2, np.uint8)), dict(out=np.zeros((3, 71), np.float32)), dict(dropout=2.0)):
        args = {**dict(rows=rows, n_beams=64, n_mid=8), **kw}
        with pytest.raises(ValueError):
            S.host_sensor_apply(st, args.pop("rows"), args.pop("n_beams"), args.pop("n_mid"), **args)
    buf = np.zeros((3, 200), np.float32)
    with pytest.raises(ValueError, match="overlaps"):
        S.host_sensor_apply(st, buf[:, :72], 64, 8, out=buf[:, 40:112])
    with pytest.raises(ValueError):
        S.host_sensor_apply({**st, "params": np.zeros((3, 9), np.float32)}, rows, 64, 8)


def test_vector_env_and_trainer_refuse_bad_arguments():
    """F110VectorEnv(sensor_ranges=...) and VectorTrainer(sensor_ranges=...) with bad values, and the
    --sensor-* flags: ValueError before anything is built (host values only: no GPU)."""
    import argparse
    from f110_gymnasium_ros2_jazzy_amd import train
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    for bad in ({"noise": (0, 0.1)}, {"noise_abs": (0.2, 0.1)}, {"dropout": (0, 1.5)}, {"scale": (0, 1)},
                {"blackout": (0, 2000)}, {"quant": -1}, {"pose_xy": (-1, 0)}, [("noise_abs", (0, 1))], 0.1):
        with pytest.raises(ValueError):
            F110VectorEnv(2, num_agents=2, sensor_ranges=bad)
        with pytest.raises(ValueError):
            train.VectorTrainer(4, sensor_ranges=bad)
    with pytest.raises(ValueError, match="unknown"):
        F110VectorEnv(2, num_agents=2, sensor_ranges={"noise": (0, 0.1)})
    with pytest.raises(ValueError):  # a sector wider than this env's beams
        F110VectorEnv(2, num_agents=2, sensor_ranges={"blackout": (0, 101)}, num_beams=100)
    ok = {"noise_abs": (0.0, 0.03)}
    for kw in (dict(sensor_mask=np.ones(3, np.uint8)), dict(sensor_mask=np.ones(2)), dict(sensor_mask="all")):
        with pytest.raises(ValueError):
            F110VectorEnv(2, num_agents=2, sensor_ranges=ok, **kw)
    for kw in (dict(sensor_seed=3), dict(sensor_mask=np.ones(2, np.uint8))):
        with pytest.raises(ValueError, match="sensor_ranges"):
            F110VectorEnv(2, num_agents=2, **kw)
    with pytest.raises(ValueError, match="sensor_ranges"):
        train.VectorTrainer(4, sensor_seed=3)
    ap = argparse.ArgumentParser()
    train.add_sensor_args(ap)
    assert train.sensor_ranges_from_args(ap.parse_args([])) is None
    args = ap.parse_args(["--sensor-noise", "0.005,0.03", "--sensor-noise-rel", "0,0.01", "--sensor-scale", "0.98,1.02",
                          "--sensor-dropout", "0,0.02", "--sensor-blackout", "0,30", "--sensor-quant", "0,0.01",
                          "--sensor-pose-xy", "0,0.05", "--sensor-pose-theta", "0,0.02"])
    assert train.sensor_ranges_from_args(args) == dict(
        noise_abs=(0.005, 0.03), noise_rel=(0.0, 0.01), scale=(0.98, 1.02), dropout=(0.0, 0.02), blackout=(0.0, 30.0),
        quant=(0.0, 0.01), pose_xy=(0.0, 0.05), pose_theta=(0.0, 0.02))
    for bad in ("0.1", "a,b", "0,1,2"):
        with pytest.raises(ValueError, match="LO,HI"):
            train.sensor_ranges_from_args(ap.parse_args(["--sensor-dropout", bad]))
