"""The track observation, host side (no GPU): f110_host_track_obs -- the statement of
f110_track_obs over host arrays -- against a NumPy restatement of the row rule (projection:
oracle/reward_oracle.py's TrackOracle) on the Spielberg centerline and the four small tracks, the
named corner cases of the rule, and every argument error."""
import ctypes
import math

import numpy as np
import pytest

import pursuit_cases as C
import track_obs_cases as K

TRACKS = ["spielberg", "open4", "triangle", "repeated", "cluster"]


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def TO():
    from f110_gymnasium_ros2_jazzy_amd import track_obs
    return track_obs


@pytest.fixture(scope="module")
def cases():
    """name -> (host-only CenterlineTrack, TrackOracle, poses float32 [M, 3]); built once."""
    import reward_oracle as R
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    out = {}
    xy, _, _ = C.spielberg_xy()
    named = {"spielberg": (xy, True), **C.small_tracks()}
    for name, (pts, closed) in named.items():
        T = R.TrackOracle(pts, closed=closed)
        tr = CenterlineTrack(pts, closed=closed, device=None)
        poses = C.track_poses(T, lookahead=1.0, spread=3.0 if name == "spielberg" else 1.5)
        out[name] = (tr, T, poses)
    yield out
    for tr, _, _ in out.values():
        tr.close()


def previews(name, n):
    """The preview distances of a case: the small tracks are shorter than 8 m ahead allows."""
    scale = 1.0 if name == "spielberg" else 0.25
    return tuple(d * scale for d in K.PREVIEWS[n])


def test_exports_defaults_width(F, TO):
    L = F.load()
    for n in ("f110_default_track_obs_params", "f110_track_obs_width", "f110_track_obs", "f110_ctx_track_obs",
              "f110_host_track_obs"):
        assert n in F.EXPORTS and hasattr(L, n)
    p = TO.track_obs_params()
    assert ctypes.sizeof(p) == 120
    got = {k: getattr(p, k) for k in K.DEFAULTS if k != "preview"}
    assert got == {k: v for k, v in K.DEFAULTS.items() if k != "preview"}
    assert p.n_preview == 4 and tuple(p.preview)[:4] == K.DEFAULTS["preview"] and tuple(p.preview)[4:] == (0.0,) * 4
    for n in range(9):
        for has in (False, True):
            w = TO.track_obs_width(n, has)
            assert w == K.width(n, has) and w % 4 == 0 and 0 <= w - (7 + 2 * n + 3 * has) < 4
    assert TO.track_obs_width(4, True) == 20 and TO.track_obs_width(4, False) == 16 and TO.track_obs_width(0) == 8
    assert L.f110_track_obs_width(9, 0) == -1 and L.f110_track_obs_width(-1, 1) == -1
    with pytest.raises(ValueError):
        TO.track_obs_width(9)
    with pytest.raises(ValueError, match="unknown"):
        TO.track_obs_params(lookahead=1.0)
    with pytest.raises(ValueError):
        TO.track_obs_params(direction=0)
    with pytest.raises(ValueError):
        TO.track_obs_params(preview=range(1, 10))
    q = TO.track_obs_params(preview=[0.5, 3.0], gap_scale=5.0, direction=-1)
    assert (q.n_preview, q.preview[0], q.preview[1], q.preview[2], q.gap_scale, q.direction) == (2, 0.5, 3.0, 0.0, 5.0, -1)
    low, high = TO.track_obs_columns(4, True)
    assert np.flatnonzero(np.isfinite(low)).tolist() == [5, 6, 15] and (high[[5, 6, 15]] == 1.0).all()
    assert np.flatnonzero(np.isfinite(TO.track_obs_columns(2, False)[1])).tolist() == [5, 6]


@pytest.mark.parametrize("name", TRACKS)
def test_matches_restatement(F, TO, cases, name):
    tr, T, poses = cases[name]
    L = F.load()
    assert np.array_equal(tr.s, T.s) and tr.L == T.L and np.array_equal(tr.tan, T.tan)
    n = 0
    for E in K.ENVS:
        for A, seat, other in K.SEATS:
            st = K.states_from_poses(poses, E, A, seed=n)
            for direction in (1, -1):
                for npv in (0, 4, 8):
                    kw = dict(preview=previews(name, npv), direction=direction)
                    want = K.np_track_obs(L, T, st, E, A, seat, other, **kw)
                    got = TO.host_track_obs(st, tr, E, A, seat, other, **kw)
                    assert got.shape == (E, K.width(npv, other is not None)) and got.shape[1] % 4 == 0
                    K.assert_rows_close(got, want, (name, E, A, seat, other, kw))
                    pad = 7 + 2 * npv + (3 if other is not None else 0)
                    assert (got[:, pad:].view(np.uint32) == 0).all()  # the pad columns: +0
                    assert (np.abs(got[:, 5:7]) <= 1.0 + 1e-6).all()
                    if name in ("spielberg", "open4", "triangle"):  # (a zero-length segment's tangent is 0)
                        assert np.allclose(got[:, 5] ** 2 + got[:, 6] ** 2, 1.0, atol=1e-5)  # sine and cosine
                    n += 1
    # other scales
    kw = dict(v_scale=8.0, steer_scale=0.3, yaw_rate_scale=3.0, slip_scale=0.5, lat_scale=1.5, gap_scale=2.0,
              preview=previews(name, 4))
    st = K.states_from_poses(poses, 65, 2, seed=99)
    K.assert_rows_close(TO.host_track_obs(st, tr, 65, 2, 0, 1, **kw), K.np_track_obs(L, T, st, 65, 2, 0, 1, **kw), name)


def test_own_columns_by_hand(F, TO, cases):
    """A car on open4's first segment (along +x): the columns read off by hand."""
    tr, T, _ = cases["open4"]
    st = K.state_of([(1.0, 0.5, math.pi / 2, 5.0, 0.2, -1.0, 0.1)])
    row = TO.host_track_obs(st, tr, 1, 1, preview=(1.0, 2.0))[0]
    assert row.shape == (12,)
    want = [5.0 / 20.0, 0.2 / 0.4189, -0.1, 0.1 / (math.pi / 3), 0.5, 1.0, 0.0,  # heading 90 deg left of the tangent
            -0.5, -1.0, -0.25, -1.0, 0.0]  # the points at s = 2 and 3, in the car's frame, over d
    assert np.allclose(row, want, atol=1e-6)
    assert row[6] == 0.0 or abs(row[6]) < 1e-16
    rev = TO.host_track_obs(st, tr, 1, 1, preview=(1.0,), direction=-1)[0]
    assert np.allclose(rev[:9], [0.25, 0.2 / 0.4189, -0.1, 0.1 / (math.pi / 3), -0.5, -1.0, 0.0, -0.5, 1.0], atol=1e-6)


def test_preview_wraps_on_a_closed_track(F, TO, cases):
    tr, T, _ = cases["spielberg"]
    L = F.load()
    cars = []
    for s_at in (T.L - 0.3, T.L - 3.9, 0.2, 3.0):  # within the preview of the seam, from both sides
        i = T.seg_at(s_at)
        p = T.xy[i] + (s_at - T.s[i]) / (T.s[i + 1] - T.s[i]) * (T.xy[i + 1] - T.xy[i])
        cars.append((np.float32(p[0]), np.float32(p[1]), np.float32(math.atan2(T.tan[i, 1], T.tan[i, 0])), 3.0))
    st = K.state_of(cars)
    for direction in (1, -1):
        got = TO.host_track_obs(st, tr, 4, 1, direction=direction)
        K.assert_rows_close(got, K.np_track_obs(L, T, st, 4, 1, direction=direction), direction)
        # on the line, heading along it: every preview point lies ahead (behind when driven backwards)
        # whichever side of the seam it falls on
        assert (got[:, 7:15:2] * direction > 0.5).all(), got[:, 7:15:2]
    s = [K.project(T, *c[:2])[0] for c in cars]
    assert s[0] + 1.0 > T.L and s[1] + 4.0 > T.L > s[1] + 2.0 and s[2] - 1.0 < 0.0 and s[3] - 4.0 < 0.0 < s[3] - 2.0


def test_preview_clamps_on_an_open_track(F, TO, cases):
    tr, T, _ = cases["open4"]
    L = F.load()
    st = K.state_of([(11.5, 2.0, 0.0, 2.0), (0.5, 0.0, 0.0, 2.0)])
    kw = dict(preview=(0.25, 1.0, 2.0))
    fwd = TO.host_track_obs(st, tr, 2, 1, **kw)
    K.assert_rows_close(fwd, K.np_track_obs(L, T, st, 2, 1, **kw))
    # 0.5 m before the end: the points 1 and 2 m ahead are the last node, 0.5 m ahead
    assert np.allclose(fwd[0, 7:13], [1.0, 0.0, 0.5 / 1.0, 0.0, 0.5 / 2.0, 0.0], atol=1e-6)
    bwd = TO.host_track_obs(st, tr, 2, 1, direction=-1, **kw)
    K.assert_rows_close(bwd, K.np_track_obs(L, T, st, 2, 1, direction=-1, **kw))
    # 0.5 m after the start, driven backwards: clamped to the first node, 0.5 m behind the car's nose
    assert np.allclose(bwd[1, 7:13], [-1.0, 0.0, -0.5 / 1.0, 0.0, -0.5 / 2.0, 0.0], atol=1e-6)


def test_cluster_fallback_node(F, TO, cases):
    """Near the cluster all five nearest midpoints belong to zero-length segments and the projection
    falls back to the nearest node (t = 0)."""
    tr, T, _ = cases["cluster"]
    L = F.load()
    st = K.state_of([(4.0, 0.1, 0.3, 1.0), (4.05, -0.2, -1.0, 2.0)])
    assert all(K.project(T, *st[:2, c])[1:] == (0.0, 2) for c in range(2))  # fallback: t = 0, the first copy
    for direction in (1, -1):
        kw = dict(preview=(0.5, 1.0), direction=direction)
        K.assert_rows_close(TO.host_track_obs(st, tr, 1, 2, 0, 1, **kw), K.np_track_obs(L, T, st, 1, 2, 0, 1, **kw))


def test_fallback_returns_last_node(F, TO):
    """The fallback's node can be the last one, seg = n-1, which has no segment of its own: the
    tangent is segment n-2's."""
    import reward_oracle as R
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    # every segment but the first is shorter than 1e-6 (L2 <= 1e-12), so near the far end all five nearest
    # midpoints are degenerate and the nearest node wins: node n-1, the only one at x = 1e-7 * 6
    pts = np.array([[-50.0, 0.0]] + [[k * 1e-7, 0.0] for k in range(7)])
    T, tr = R.TrackOracle(pts, closed=False), CenterlineTrack(pts, closed=False, device=None)
    try:
        st = K.state_of([(1.0, 0.0, 0.1, 2.0), (2.0, 0.5, 0.0, 1.0)])
        assert K.project(T, 1.0, 0.0)[2] == T.n - 1 and K.project(T, 2.0, 0.5)[2] == T.n - 1
        for kw in (dict(preview=(0.5, 20.0)), dict(preview=(0.5, 20.0), direction=-1)):
            got = TO.host_track_obs(st, tr, 1, 2, 0, 1, **kw)
            K.assert_rows_close(got, K.np_track_obs(F.load(), T, st, 1, 2, 0, 1, **kw), kw)
            assert np.isfinite(got).all() and got[0, 4] == 0.0
            # the tangent of segment n-2 (along +x): heading 0.1 rad left of it
            assert np.allclose(got[0, 5:7], [kw.get("direction", 1) * math.sin(0.1), kw.get("direction", 1) * math.cos(0.1)],
                               atol=1e-6)
    finally:
        tr.close()


def test_gap_wraps_and_clips(F, TO, cases):
    tr, T, _ = cases["spielberg"]
    L = F.load()

    def at(s_at, v):
        i = T.seg_at(s_at)
        p = T.xy[i] + (s_at - T.s[i]) / (T.s[i + 1] - T.s[i]) * (T.xy[i + 1] - T.xy[i])
        return (np.float32(p[0]), np.float32(p[1]), np.float32(math.atan2(T.tan[i, 1], T.tan[i, 0])), v)

    half = 0.5 * T.L
    # env 0: the other 3 m ahead across the seam; 1: 3 m behind across it; 2 / 3: just short of and just
    # past half a lap ahead (the gap's sign flips); 4: 25 m ahead (clipped to +1); 5: 25 m behind (-1)
    pairs = [(T.L - 1.0, 2.0), (1.0, T.L - 2.0), (10.0, 10.0 + half - 0.5), (10.0, 10.0 + half + 0.5),
             (100.0, 125.0), (100.0, 75.0)]
    st = K.state_of([c for a, b in pairs for c in (at(a, 4.0), at(b, 6.5))])
    for direction in (1, -1):
        got = TO.host_track_obs(st, tr, 6, 2, 0, 1, gap_scale=10.0, direction=direction)
        want = K.np_track_obs(L, T, st, 6, 2, 0, 1, gap_scale=10.0, direction=direction)
        K.assert_rows_close(got, want, direction)
        g = got[:, 15].astype(np.float64) * direction
        assert abs(g[0] - 0.3) < 1e-3 and abs(g[1] + 0.3) < 1e-3, g
        assert g[2] == 1.0 and g[3] == -1.0  # +-(L/2 - 0.5) m, clipped, the sign from the wrap
        assert g[4] == 1.0 and g[5] == -1.0
        assert np.allclose(got[:, 17], 2.5 / 20.0)
    # unclipped around the half lap: a gap scale of a whole lap
    got = TO.host_track_obs(st, tr, 6, 2, 0, 1, gap_scale=T.L)
    assert abs(got[2, 15] - (half - 0.5) / T.L) < 1e-4 and abs(got[3, 15] + (half - 0.5) / T.L) < 1e-4
    K.assert_rows_close(got, K.np_track_obs(L, T, st, 6, 2, 0, 1, gap_scale=T.L))
    # seen from the other seat the gap changes sign
    back = TO.host_track_obs(st, tr, 6, 2, 1, 0, gap_scale=T.L)
    assert np.allclose(back[:2, 15], -got[:2, 15], atol=1e-6) and np.allclose(back[:, 17], -2.5 / 20.0)


def test_non_finite_poses(F, TO, cases):
    tr, T, poses = cases["spielberg"]
    L = F.load()
    st = K.states_from_poses(poses, 8, 2, seed=5)
    st[0, 0] = np.nan         # env 0: the seat's x
    st[1, 2] = np.inf         # env 1: the seat's y
    st[4, 4] = -np.inf        # env 2: the seat's yaw
    st[0, 7] = np.nan         # env 3: the other's x
    st[1, 9] = -np.inf        # env 4: the other's y
    st[4, 11] = np.nan        # env 5: the other's yaw does not enter
    got = TO.host_track_obs(st, tr, 8, 2, 0, 1)
    want = K.np_track_obs(L, T, st, 8, 2, 0, 1)
    K.assert_rows_close(got, want)
    assert (got[:3].view(np.uint32) == 0).all()  # all-zero rows, +0
    assert (got[3:5, 15:18].view(np.uint32) == 0).all() and (got[3:5, :15] != 0).any(axis=1).all()
    clean = K.states_from_poses(poses, 8, 2, seed=5)
    ref = TO.host_track_obs(clean, tr, 8, 2, 0, 1)
    K.assert_rows_equal(got[3:5, :15], ref[3:5, :15])  # the rest of the row is intact
    K.assert_rows_equal(got[5:], ref[5:])
    # a non-finite speed is no pose: it goes through to its column
    st2 = clean.copy()
    st2[3, 0] = np.nan
    assert np.isnan(TO.host_track_obs(st2, tr, 8, 2, 0, 1)[0, [0, 17]]).all()


def test_strided_rows_keep_their_neighbours(F, TO, cases):
    tr, T, poses = cases["spielberg"]
    st = K.states_from_poses(poses, 5, 2, seed=3)
    want = TO.host_track_obs(st, tr, 5, 2, 0, 1)
    sentinel = np.float32(-7.25)
    buf = np.full((5, 11 + 20 + 6), sentinel)
    got = TO.host_track_obs(st, tr, 5, 2, 0, 1, out=buf[:, 11:31])
    assert np.shares_memory(got, buf)
    K.assert_rows_equal(buf[:, 11:31], want)
    assert (buf[:, :11] == sentinel).all() and (buf[:, 31:] == sentinel).all()
    with pytest.raises(ValueError):
        TO.host_track_obs(st, tr, 5, 2, 0, 1, out=buf[:, 11:30])


def test_invalid_arguments(F, TO, cases):
    L = F.load()
    tr, T, poses = cases["open4"]  # L = 12.47 m
    st = K.states_from_poses(poses, 3, 2)
    out = np.zeros((3, 20), np.float32)

    def call(track=tr.handle, state=st.ctypes.data, n_envs=3, n_agents=2, seat=0, other=1, o=out.ctypes.data, stride=20,
             params=True, **kw):
        p = TO.track_obs_params(preview=(0.5, 1.0, 2.0, 3.0))
        for k, v in kw.items():
            if k == "preview":
                for j, d in enumerate(v):
                    p.preview[j] = d
            else:
                setattr(p, k, v)
        return L.f110_host_track_obs(track, ctypes.byref(p) if params else None, state, n_envs, n_agents, seat, other,
                                     o, stride)

    assert call() == 0
    nan = float("nan")
    bad = [dict(track=None), dict(params=False), dict(state=None), dict(o=None), dict(n_envs=-1), dict(n_agents=0),
           dict(n_agents=9), dict(seat=-1), dict(seat=2), dict(other=-2), dict(other=2), dict(other=0), dict(stride=19),
           dict(n_preview=-1), dict(n_preview=9), dict(direction=0), dict(direction=2),
           dict(preview=(0.0,)), dict(preview=(-1.0,)), dict(preview=(0.5, T.L)), dict(preview=(0.5, 1.0, 2.0, 1e9)),
           dict(preview=(nan,))]
    for f in ("v_scale", "steer_scale", "yaw_rate_scale", "slip_scale", "lat_scale", "gap_scale"):
        bad += [{f: 0.0}, {f: -1.0}, {f: nan}]
    for kw in bad:
        out[:] = 3.0
        assert call(**kw) == -1, kw  # F110_E_INVALID
        assert L.f110_last_error(), kw
        assert (out == 3.0).all(), kw
    # an unused preview distance is not looked at; n_envs = 0 is an empty call
    assert call(n_preview=2, preview=(0.5, 1.0, -5.0, nan), stride=16) == 0
    assert call(n_envs=0) == 0
    # without another car the width is smaller, and so is the smallest stride
    assert call(other=-1, stride=16) == 0 and call(other=-1, stride=15) == -1
    # the device entries refuse a host-only track by name
    p = TO.track_obs_params(preview=(0.5,))
    assert L.f110_track_obs(tr.handle, ctypes.byref(p), st.ctypes.data, 3, 2, 0, 1, out.ctypes.data, 20, None) == -1
    assert b"device track" in L.f110_last_error()
    assert L.f110_ctx_track_obs(None, tr.handle, ctypes.byref(p), 0, 1, out.ctypes.data, 20, None) == -1
    assert L.f110_last_error()
    # the Python wrappers' own checks
    for kw in (dict(seat=2), dict(other=0), dict(other=5), dict(seat=-1)):
        with pytest.raises(ValueError):
            TO.host_track_obs(st, tr, 3, 2, **{"seat": 0, **kw})
    with pytest.raises(ValueError):
        TO.host_track_obs(st[:, :5], tr, 3, 2)
    with pytest.raises(F.F110Error):
        TO.host_track_obs(st, tr, 3, 2, preview=(100.0,))


def test_vector_env_refuses_a_bad_centerline(cases):
    """F110VectorEnv(track_obs=...) without a usable device centerline: ValueError before anything
    is built (host values only, so it runs without a GPU)."""
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    tr, _, _ = cases["spielberg"]  # host-only
    with pytest.raises(ValueError, match="centerline"):
        F110VectorEnv(2, num_agents=2, track_obs=True)
    with pytest.raises(ValueError, match="centerline"):
        F110VectorEnv(2, num_agents=2, track_obs=True, obs_track=tr)
    with pytest.raises(ValueError, match="unknown"):
        F110VectorEnv(2, num_agents=2, track_obs={"lookahead": 1.0}, obs_track=tr)
