"""The scan observation, host side (no GPU): f110_host_scan_obs_push -- the statement of
f110_scan_obs_push over host arrays -- against a NumPy restatement of the row rule
(tests/scan_obs_cases.py) over sequences of pushes with resets in the middle, the known answers of
the ring, the width function, and every argument error.  Bit-for-bit equality throughout."""
import ctypes

import numpy as np
import pytest

import scan_obs_cases as C


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def SO():
    from f110_gymnasium_ros2_jazzy_amd import scan_obs
    return scan_obs


def run_sequence(SO, B, K, F_, S, reduce, N, M, T, keep_mid, strided, seed):
    """2*D + 3 pushes of N envs through the library's host statement and the restatement, with
    per-env reset flags in the middle; every push's rows, ring and head are compared."""
    rng = np.random.default_rng(seed)
    D = C.depth(F_, S)
    kw = dict(n_bins=K, n_frames=F_, stride=S, reduce=reduce, keep_mid=keep_mid)
    lib, ref = SO.host_scan_obs_state(N, B, **kw), C.fresh(N, K, F_, S)
    W = C.width(K, F_, M, T, keep_mid)
    for t in range(2 * D + 3):
        rows = C.rows_for(rng, N, B, M, T, stride=B + M + T + 5 if strided else None)
        reset = None
        if t in (D + 1, D + 2):  # some envs, then (almost surely) others, one push later
            reset = (rng.random(N) < 0.5).astype(np.uint8)
        elif t == 2:
            reset = np.zeros(N, np.uint8)  # flags given, none set
        out = np.full((N, W + 3), np.float32(-7.0)) if strided else None
        got = SO.host_scan_obs_push(lib, rows, B, M, T, reset=reset, out=None if out is None else out[:, :W], **kw)
        want = C.push(ref, rows, B, M, T, K, F_, S, reduce, keep_mid, reset)
        assert C.same_bits(got, want), (t, "rows")
        assert C.same_bits(lib["ring"], ref["ring"]) and C.same_bits(lib["head"], ref["head"]), (t, "state")
        if out is not None:
            assert (out[:, W:] == np.float32(-7.0)).all()  # the neighbours of strided rows are kept


def test_exports_defaults_width(F, SO):
    L = F.load()
    for n in ("f110_default_scan_obs_params", "f110_scan_obs_width", "f110_scan_obs_create", "f110_scan_obs_destroy",
              "f110_scan_obs_push", "f110_scan_obs_reset", "f110_scan_obs_arrays", "f110_host_scan_obs_push"):
        assert n in F.EXPORTS and hasattr(L, n)
    p = SO.scan_obs_params()
    assert ctypes.sizeof(p) == 20
    assert (p.n_bins, p.n_frames, p.stride, p.reduce, p.keep_mid) == (108, 1, 1, 0, 1)
    assert SO.scan_obs_width(1080, 8) == 116 and SO.scan_obs_width(1080, 8, 20) == 136
    assert SO.scan_obs_width(1080, 8, 20, n_bins=36, n_frames=3, stride=2) == 3 * 36 + 8 + 20
    assert SO.scan_obs_width(1080, 8, 20, n_bins=36, n_frames=3, stride=2, keep_mid=False) == 3 * 36 + 20
    assert SO.scan_obs_width(1080, 8, n_bins=1080) == 1088  # the identity keeps the row's width
    for B, K, F_, S in C.CASES + (C.DEEP,):
        for M in (4, 8):
            for T in (0, 20):
                for keep in (True, False):
                    w = SO.scan_obs_width(B, M, T, n_bins=K, n_frames=F_, stride=S, keep_mid=keep)
                    assert w == C.width(K, F_, M, T, keep)
    q = SO.scan_obs_params(n_bins=7, n_frames=3, stride=2, reduce="mean", keep_mid=False)
    assert (q.n_bins, q.n_frames, q.stride, q.reduce, q.keep_mid) == (7, 3, 2, 1, 0) and SO.scan_obs_depth(q) == 5
    lo, hi = SO.scan_obs_columns(SO.scan_obs_params(n_bins=3, n_frames=2), [-5, -6], [5, 6], [-1], [1])
    assert lo.tolist() == [0.0] * 6 + [-5.0, -6.0, -1.0] and hi.tolist() == [1.0] * 6 + [5.0, 6.0, 1.0]
    lo, hi = SO.scan_obs_columns(SO.scan_obs_params(n_bins=3, keep_mid=False), [-5, -6], [5, 6], [-1], [1])
    assert lo.tolist() == [0.0] * 3 + [-1.0] and hi.tolist() == [1.0] * 3 + [1.0] and lo.dtype == np.float32
    bad = F.F110ScanObsParams(n_bins=0, n_frames=1, stride=1, reduce=0, keep_mid=1)
    assert L.f110_scan_obs_width(ctypes.byref(bad), 1080, 8, 0) == -1
    assert L.f110_scan_obs_width(None, 1080, 8, 0) == -1
    assert L.f110_scan_obs_width(ctypes.byref(p), 107, 8, 0) == -1  # K > B
    assert L.f110_scan_obs_width(ctypes.byref(p), 1080, -1, 0) == -1


@pytest.mark.parametrize("reduce", C.REDUCES)
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: "B%d_K%d_F%d_S%d" % c)
def test_matches_restatement(SO, case, reduce):
    B, K, F_, S = case
    for i, N in enumerate(C.ENVS_HOST):  # M, T, keep_mid and the row strides vary with the env count
        M, T = (4, 8, 8)[i], (0, 20, 0)[i]
        run_sequence(SO, B, K, F_, S, reduce, N, M, T, keep_mid=i != 1, strided=i != 0, seed=100 * i + K)


@pytest.mark.parametrize("reduce", C.REDUCES)
def test_deepest_ring(SO, reduce):
    B, K, F_, S = C.DEEP
    assert C.depth(F_, S) == 31
    run_sequence(SO, B, K, F_, S, reduce, 3, 8, 20, keep_mid=True, strided=True, seed=7)


@pytest.mark.parametrize("reduce", C.REDUCES)
def test_identity_returns_the_row(SO, reduce):
    """K == B, one frame, poses kept: the output row is the input row bit for bit (a mean over one
    beam divides by 1.0f), whatever the values."""
    rng = np.random.default_rng(3)
    rows = C.rows_for(rng, 3, 1080, 8, 20)
    rows[0, :4] = [0.0, np.float32(1e-42), np.inf, 1.0]  # a zero, a subnormal, an infinity
    st = SO.host_scan_obs_state(3, 1080, n_bins=1080, reduce=reduce)
    for _ in range(2):
        assert C.same_bits(SO.host_scan_obs_push(st, rows, 1080, 8, 20, n_bins=1080, reduce=reduce), rows)


def test_ring_known_answers(SO):
    """After a refill every stacked frame is equal; after one more push only frame 0 differs when
    S == 1, and with S > 1 frame j takes a new value only S*j pushes after the refill."""
    rng = np.random.default_rng(11)
    B, M, K = 40, 4, 5
    for F_, S in ((4, 1), (3, 2), (3, 3)):
        kw = dict(n_bins=K, n_frames=F_, stride=S)
        st = SO.host_scan_obs_state(2, B, **kw)
        first = SO.host_scan_obs_push(st, C.rows_for(rng, 2, B, M, 0), B, M, **kw)
        frames = first[:, :F_ * K].reshape(2, F_, K)
        assert all(C.same_bits(frames[:, j], frames[:, 0]) for j in range(F_))
        assert (st["head"] == 0).all() and all(C.same_bits(st["ring"][:, d], frames[:, 0]) for d in range(C.depth(F_, S)))
        f0 = frames[:, 0].copy()
        history = [f0]
        for t in range(1, S * (F_ - 1) + 2):
            out = SO.host_scan_obs_push(st, C.rows_for(rng, 2, B, M, 0), B, M, **kw)
            fr = out[:, :F_ * K].reshape(2, F_, K)
            history.append(fr[:, 0].copy())
            assert not C.same_bits(fr[:, 0], f0)
            for j in range(1, F_):  # frame j is the frame pushed j*S pushes ago, the refill's before that
                assert C.same_bits(fr[:, j], history[max(t - j * S, 0)])
        # a reset flag refills one env and leaves the other's ring alone
        before = st["ring"][1].copy()
        out = SO.host_scan_obs_push(st, C.rows_for(rng, 2, B, M, 0), B, M, reset=np.array([1, 0], np.uint8), **kw)
        fr = out[:, :F_ * K].reshape(2, F_, K)
        assert st["head"][0] == 0 and all(C.same_bits(fr[0, j], fr[0, 0]) for j in range(F_))
        assert F_ == 1 or not C.same_bits(fr[1, 1], fr[1, 0])
        assert (st["ring"][1] != before).any(axis=1).sum() == 1  # one slot took the frame


def test_middle_and_tail_are_the_current_rows(SO):
    rng = np.random.default_rng(5)
    B, M, T, K = 67, 8, 20, 9
    for keep in (True, False):
        kw = dict(n_bins=K, n_frames=2, stride=3, keep_mid=keep)
        st = SO.host_scan_obs_state(3, B, **kw)
        for _ in range(5):
            rows = C.rows_for(rng, 3, B, M, T)
            out = SO.host_scan_obs_push(st, rows, B, M, T, **kw)
            assert C.same_bits(out[:, 2 * K:], rows[:, B:] if keep else rows[:, B + M:])


def test_invalid_arguments(F, SO):
    L = F.load()
    rows = np.zeros((3, 1088), np.float32)
    ok = dict(n_bins=108, n_frames=1, stride=1)
    for bad in (dict(n_bins=0), dict(n_bins=1081), dict(n_frames=0), dict(n_frames=9), dict(stride=0), dict(stride=17),
                dict(n_frames=3, stride=16), dict(n_frames=8, stride=5), dict(reduce="median"), dict(reduce=2),
                dict(keep_mid=2), dict(n_bins=3.5), dict(n_bins=True), dict(bins=4)):
        with pytest.raises(ValueError):
            SO.scan_obs_params(1080, **{**ok, **bad})
    with pytest.raises(ValueError, match="unknown"):
        SO.scan_obs_params(bins=4)
    with pytest.raises(ValueError):
        SO.scan_obs_width(0, 8)
    with pytest.raises(ValueError):
        SO.scan_obs_width(4097, 8)
    with pytest.raises(ValueError):
        SO.scan_obs_width(1080, -1)
    st = SO.host_scan_obs_state(3, 1080)
    with pytest.raises(ValueError):  # the rows' width
        SO.host_scan_obs_push(st, rows[:, :1087], 1080, 8)
    with pytest.raises(ValueError):  # the state's shape
        SO.host_scan_obs_push(st, rows, 1080, 8, n_bins=36)
    with pytest.raises(ValueError):  # the flags' length
        SO.host_scan_obs_push(st, rows, 1080, 8, reset=np.zeros(2, np.uint8))
    with pytest.raises(ValueError):  # out's width
        SO.host_scan_obs_push(st, rows, 1080, 8, out=np.zeros((3, 115), np.float32))
    with pytest.raises(ValueError):  # float64 rows
        SO.host_scan_obs_push(st, rows.astype(np.float64), 1080, 8)
    buf = np.zeros((3, 1300), np.float32)
    with pytest.raises(ValueError, match="overlaps"):  # out inside the rows' span
        SO.host_scan_obs_push(st, buf[:, :1088], 1080, 8, out=buf[:, 1100:1216])
    st["head"][1] = 1  # D = 1: no such slot
    with pytest.raises(ValueError, match="head"):
        SO.host_scan_obs_push(st, rows, 1080, 8)
    st["head"][1] = -1
    # the C entry itself: every refusal is F110_E_INVALID with a message
    p = SO.scan_obs_params()
    out = np.zeros((3, 116), np.float32)
    ring, head = np.zeros((3, 1, 108), np.float32), np.full(3, -1, np.int32)

    def call(params=p, n=3, B=1080, M=8, T=0, r=rows, rs=1088, rg=ring, h=head, o=out, os_=116):
        a = [None if x is None else x.ctypes.data for x in (r, rg, h, o)]
        return L.f110_host_scan_obs_push(None if params is None else ctypes.byref(params), n, B, M, T, a[0], rs, None,
                                         a[1], a[2], a[3], os_)
    assert call() == 0
    q = F.F110ScanObsParams(n_bins=109, n_frames=1, stride=1, reduce=0, keep_mid=1)
    for kw in (dict(params=None), dict(n=0), dict(B=0), dict(B=4097), dict(M=-1), dict(T=-1), dict(r=None), dict(rg=None),
               dict(h=None), dict(o=None), dict(rs=1087), dict(os_=115), dict(o=rows), dict(params=q, B=108, rs=116)):
        assert call(**kw) == -1, kw
        assert b"f110_host_scan_obs_push" in L.f110_last_error()
    for f, s in ((9, 1), (0, 1), (1, 0), (1, 17), (3, 16)):
        q = F.F110ScanObsParams(n_bins=108, n_frames=f, stride=s, reduce=0, keep_mid=1)
        assert call(params=q) == -1
    for red, keep in ((2, 1), (-1, 1), (0, 2)):
        q = F.F110ScanObsParams(n_bins=108, n_frames=1, stride=1, reduce=red, keep_mid=keep)
        assert call(params=q) == -1


def test_vector_env_and_trainer_refuse_bad_arguments():
    """F110VectorEnv(scan_obs=...) and VectorTrainer(scan_*=...) with bad values: ValueError before
    anything is built (host values only, so it runs without a GPU)."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    for bad in ({"bins": 36}, {"n_bins": 0}, {"n_bins": 1081}, {"n_frames": 9}, {"stride": 17},
                {"n_frames": 3, "stride": 16}, {"reduce": "max"}, 36, "min"):
        with pytest.raises(ValueError):
            F110VectorEnv(2, num_agents=2, scan_obs=bad)
    with pytest.raises(ValueError, match="unknown"):
        F110VectorEnv(2, num_agents=2, scan_obs={"bins": 36})
    with pytest.raises(ValueError):  # more sectors than this env's beams
        F110VectorEnv(2, num_agents=2, scan_obs={"n_bins": 108}, num_beams=100)
    for bad in (dict(scan_frames=2), dict(scan_stride=2), dict(scan_reduce="mean"), dict(scan_keep_poses=False),
                dict(scan_bins=0), dict(scan_bins=2000), dict(scan_bins=36, scan_frames=9),
                dict(scan_bins=36, scan_frames=3, scan_stride=16), dict(scan_bins=36, scan_reduce="max"),
                dict(scan_bins=36.5)):
        with pytest.raises(ValueError):
            VectorTrainer(4, **bad)
    with pytest.raises(ValueError, match="scan_bins"):
        VectorTrainer(4, scan_frames=2)
