"""What tests/test_pursuit_host.py and tests/test_gpu_pursuit.py share: the tracks and poses the
pure-pursuit opponent is checked on, its NumPy restatement over oracle/reward_oracle.py's
TrackOracle, the float32-ulp comparison of actions, and the closed-loop spawn layout."""
import ctypes
import math
import os

import numpy as np

from conftest import MAPS

DEFAULTS = dict(lookahead=1.2, wheelbase=0.3302, speed=4.0, a_lat=0.0, v_floor=1.0, steer_limit=0.4189, direction=1)
ROWS = (1, 2, 3, 65)  # one half-wave, one wave, an odd tail, more than one block


def spielberg_xy():
    with np.load(os.path.join(MAPS, "Spielberg_centerline.npz")) as z:
        return z["xy"].copy(), z["w_right"].copy(), z["w_left"].copy()


def small_tracks():
    """name -> (xy, closed): an open 4-point track, a closed triangle (3 segments: fewer than the 5
    candidates), a track with one repeated point (a segment with L2 <= 1e-12) and one with a
    cluster of them.  Coordinates are float32-exact so that a float32 pose can sit exactly on a
    node."""
    return {
        "open4": (np.array([[0.0, 0.0], [4.0, 0.0], [8.0, 2.0], [12.0, 2.0]]), False),
        "triangle": (np.array([[0.0, 0.0], [4.0, 0.0], [2.0, 3.0], [0.0, 0.0]]), True),
        "repeated": (np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 0.0], [6.0, 1.0], [9.0, 1.0], [12.0, 0.0]]), False),
        # six copies of one node: near it the 5 nearest midpoints all belong to zero-length segments,
        # and the projection falls back to the nearest node
        "cluster": (np.array([[0.0, 0.0], [2.0, 0.0]] + [[4.0, 0.0]] * 6 + [[6.0, 0.0], [8.0, 1.0]]), False),
    }


def track_poses(T, lookahead=1.2, seed=0, spread=3.0):
    """float32 poses [M, 3] on TrackOracle T: on the centerline (tangent heading), up to +-spread m
    off it with random headings, 100 m away, within `lookahead` of both ends of s (the wrap / the
    open-track clamp), on the nodes themselves, and a tie between two midpoints."""
    rng = np.random.default_rng(seed + T.n)
    rows = []
    k = np.unique(np.linspace(0, T.n - 2, 12).astype(int))
    th = np.arctan2(T.tan[k, 1], T.tan[k, 0])
    rows.append(np.c_[T.xy[k], th])                                   # on the centerline
    rows.append(np.c_[T.mid[k], th + 0.3])                            # on a midpoint, heading off the tangent
    off = rng.uniform(-spread, spread, (len(k), 2))
    rows.append(np.c_[T.xy[k] + off, rng.uniform(-np.pi, np.pi, len(k))])  # off the line
    c = T.xy.mean(axis=0)
    rows.append(np.array([[c[0] + 100.0, c[1] - 100.0, 0.5], [c[0] - 100.0, c[1] + 70.0, -2.0]]))  # off the grid
    for s_at in (0.0, 0.25 * lookahead, 0.9 * lookahead, T.L - 0.9 * lookahead, T.L - 0.25 * lookahead, T.L):
        i = T.seg_at(s_at)
        seg = T.s[i + 1] - T.s[i]
        u = 0.0 if seg == 0 else (s_at - T.s[i]) / seg
        p = T.xy[i] + u * (T.xy[i + 1] - T.xy[i])
        rows.append(np.array([[p[0], p[1], math.atan2(T.tan[i, 1], T.tan[i, 0])],
                              [p[0] + 0.2, p[1] - 0.1, math.atan2(T.tan[i, 1], T.tan[i, 0]) + 3.0]]))
    rows.append(np.c_[T.xy[[0, -1]], [0.1, -0.1]])                    # the end nodes (open: the last is its own target)
    rows.append(np.array([[c[0], c[1], 1.0]]))                        # the centroid (triangle: equidistant midpoints)
    return np.concatenate(rows).astype(np.float32)


def special_poses():
    """Rows with a non-finite entry (the action is (0, 0))."""
    return np.array([[np.nan, 1.0, 0.0], [1.0, np.inf, 0.0], [1.0, 1.0, -np.inf], [np.nan, np.nan, np.nan],
                     [-np.inf, 2.0, np.nan]], np.float32)


def host_sincos(L, yaw):
    """cr_sincos of one Python float through the library's host copy."""
    x = np.array([yaw], np.float64)
    sn, cs = np.empty(1), np.empty(1)
    L.f110_host_sincos(x.ctypes.data, 1, sn.ctypes.data, cs.ctypes.data)
    return float(sn[0]), float(cs[0])


def np_pursuit(L, T, poses, row_speed=None, **params):
    """Steps 1-12 of the controller (include/f110.h, "pure-pursuit opponent") in Python floats, with
    TrackOracle.project_xy / seg_at for the projection.  Returns (actions float32 [M, 2], aux [M, 4])."""
    P = {**DEFAULTS, **params}
    M = len(poses)
    act = np.zeros((M, 2), np.float32)
    aux = np.full((M, 4), np.nan)
    for m in range(M):
        x, y, yaw = (float(v) for v in poses[m, :3])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
            continue
        s_proj, t = T.project_xy(x, y)
        sq = s_proj + P["direction"] * P["lookahead"]
        if T.closed:
            if sq > T.L:
                sq -= T.L
            if sq < 0.0:
                sq += T.L
        else:
            sq = min(max(sq, 0.0), T.L)
        i = T.seg_at(sq)
        seg = float(T.s[i + 1] - T.s[i])
        u = 0.0 if seg == 0.0 else (sq - float(T.s[i])) / seg
        ax, ay = float(T.xy[i, 0]), float(T.xy[i, 1])
        tx = ax + u * (float(T.xy[i + 1, 0]) - ax)
        ty = ay + u * (float(T.xy[i + 1, 1]) - ay)
        dx, dy = tx - x, ty - y
        d2 = dx * dx + dy * dy
        sn, cs = host_sincos(L, yaw)
        ly = -sn * dx + cs * dy
        kappa = 2.0 * ly / d2 if d2 != 0.0 else math.nan  # (0 / 0)
        steer = math.atan(P["wheelbase"] * kappa)
        steer = min(max(steer, -P["steer_limit"]), P["steer_limit"]) if steer == steer else steer
        v = P["speed"] if row_speed is None else float(row_speed[m])
        if P["a_lat"] > 0.0:
            ak = abs(kappa)
            ak = ak if ak > 1e-9 else 1e-9
            v = min(max(math.sqrt(P["a_lat"] / ak), P["v_floor"]), v)
        if d2 <= 1e-12:
            steer = 0.0
        act[m] = (np.float32(steer), np.float32(v))
        aux[m] = (s_proj, t, tx, ty)
    return act, aux


def assert_actions_close(got, want, what=""):
    """float32 actions equal within one float32 ulp of the expected value or 1e-12 absolute,
    whichever is larger: the f64 atan is the one operation whose last bit libm, NumPy and ocml may
    round differently, it is well conditioned, so the float32 rounding moves by at most one ulp."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    tol = np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-12)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = ~(err <= tol) & ~np.isnan(want)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def assert_aux_equal(got, want, what=""):
    """Bit for bit (NaN rows: NaN in both)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    same = (got.view(np.uint64) == want.view(np.uint64)) | nan
    assert same.all(), (what, np.argwhere(~same)[:5].tolist(), got[~same][:5], want[~same][:5])


def lap_spawns(T, n_envs=8, lead=200):
    """Poses [n_envs, 2, 3] on the centerline at evenly spaced points, tangent headings, the ego
    (agent 0) `lead` points ahead of the opponent (agent 1)."""
    opp = (np.arange(n_envs) * ((T.n - 1) // n_envs)) % (T.n - 1)
    ego = (opp + lead) % (T.n - 1)
    k = np.stack([ego, opp], axis=1)
    return np.concatenate([T.xy[k], np.arctan2(T.tan[k, 1], T.tan[k, 0])[..., None]], axis=2)


class Progress:
    """Centerline progress (the sum of wrapped arclength steps) and the largest |t| of a set of
    cars, fed one aux block per step."""

    def __init__(self, T, n):
        self.T, self.prev, self.total, self.max_t = T, None, np.zeros(n), 0.0

    def update(self, aux):
        s = np.asarray(aux[:, 0], np.float64)
        if self.prev is not None:
            ds = s - self.prev
            ds = np.where(ds > 0.5 * self.T.L, ds - self.T.L, ds)
            ds = np.where(ds < -0.5 * self.T.L, ds + self.T.L, ds)
            self.total += ds
        self.prev = s
        self.max_t = max(self.max_t, float(np.abs(aux[:, 1]).max()))


def c_params(F, **params):
    from f110_gymnasium_ros2_jazzy_amd import opponent
    p = opponent.pursuit_params()
    for k, v in params.items():  # (no checks: the error tests need bad values)
        setattr(p, k, int(v) if k == "direction" else float(v))
    return p


NULL = ctypes.c_void_p(None)
