"""What tests/test_track_obs_host.py and tests/test_gpu_track_obs.py share: the NumPy / Python-float
restatement of the track observation's row rule (include/f110.h, "track observation") over
oracle/reward_oracle.py's TrackOracle and pursuit_cases.host_sincos, the state sets the rule is
checked on, and the comparisons."""
import math

import numpy as np

import pursuit_cases as C

DEFAULTS = dict(v_scale=20.0, steer_scale=0.4189, yaw_rate_scale=10.0, slip_scale=math.pi / 3, lat_scale=1.0,
                gap_scale=10.0, preview=(1.0, 2.0, 4.0, 8.0), direction=1)
ENVS = (1, 2, 3, 65)  # one wave, two, an odd tail of the 4-env block, more than one block
# (n_agents, seat, other)
SEATS = ((1, 0, None), (2, 0, 1), (2, 1, 0), (3, 2, 0))
PREVIEWS = {0: (), 4: (1.0, 2.0, 4.0, 8.0), 8: (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0)}


def width(n_preview, has_other):
    return (7 + 2 * n_preview + (3 if has_other else 0) + 3) // 4 * 4


def project(T, x, y):
    """TrackOracle.project_xy with the segment (or, from the fallback, the node) it took s from."""
    p = np.array([x, y], dtype=float)
    best = None
    for idx in T.nearest5(p):
        a = T.xy[idx]
        ab = T.xy[idx + 1] - a
        L2 = np.dot(ab, ab)
        if L2 <= 1e-12:
            continue
        t_par = np.clip(np.dot(p - a, ab) / L2, 0.0, 1.0)
        proj = a + t_par * ab
        cand = (np.linalg.norm(p - proj), T.s[idx] + t_par * np.linalg.norm(ab), np.dot(p - proj, T.nrm[idx]), int(idx))
        if best is None or cand[0] < best[0]:
            best = cand
    if best is None:
        j = int(np.argmin(np.linalg.norm(T.xy - p, axis=1)))
        out = float(T.s[j]), 0.0, j
    else:
        out = float(best[1]), float(best[2]), best[3]
    assert out[:2] == T.project_xy(x, y)  # the oracle's own projection, with its segment
    return out


def np_track_obs(L, T, state, n_envs, n_agents, seat=0, other=None, **params):
    """Steps 1-10 of the rule in Python floats.  state: float64 [7, E*A].  Returns float32 [E, width]."""
    P = {**DEFAULTS, **params}
    prev = [float(d) for d in P["preview"]]
    dirn = float(P["direction"])
    W = width(len(prev), other is not None)
    out = np.zeros((n_envs, W), np.float32)
    for e in range(n_envs):
        x, y, delta, v, yaw, yaw_rate, slip = (float(q) for q in state[:, e * n_agents + seat])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
            continue
        s_p, t, seg = project(T, x, y)
        i = min(seg, T.n - 2)
        sn, cs = C.host_sincos(L, yaw)
        tx, ty = dirn * float(T.tan[i, 0]), dirn * float(T.tan[i, 1])
        col = [v / P["v_scale"], delta / P["steer_scale"], yaw_rate / P["yaw_rate_scale"], slip / P["slip_scale"],
               dirn * t / P["lat_scale"], sn * tx - cs * ty, cs * tx + sn * ty]
        for d in prev:
            sq = s_p + dirn * d
            if T.closed:
                if sq > T.L:
                    sq -= T.L
                if sq < 0.0:
                    sq += T.L
            else:
                sq = min(max(sq, 0.0), float(T.L))
            k = T.seg_at(sq)
            seg_len = float(T.s[k + 1] - T.s[k])
            u = 0.0 if seg_len == 0.0 else (sq - float(T.s[k])) / seg_len
            ax, ay = float(T.xy[k, 0]), float(T.xy[k, 1])
            px = ax + u * (float(T.xy[k + 1, 0]) - ax)
            py = ay + u * (float(T.xy[k + 1, 1]) - ay)
            dx, dy = px - x, py - y
            col += [(cs * dx + sn * dy) / d, (-sn * dx + cs * dy) / d]
        if other is not None:
            xo, yo, _, vo = (float(q) for q in state[:4, e * n_agents + other])
            if math.isfinite(xo) and math.isfinite(yo):
                s_o, t_o, _ = project(T, xo, yo)
                g = dirn * (s_o - s_p)
                if T.closed:
                    if g > 0.5 * T.L:
                        g -= T.L
                    if g < -0.5 * T.L:
                        g += T.L
                g = g / P["gap_scale"]
                col += [min(max(g, -1.0), 1.0), dirn * (t_o - t) / P["lat_scale"], (vo - v) / P["v_scale"]]
        with np.errstate(over="ignore"):
            out[e, :len(col)] = np.array(col, np.float64).astype(np.float32)
    return out


def dyn_columns(M, seed):
    """Seeded (delta, v, yaw_rate, slip) [M, 4]: driving values, every fourth row the zeros a
    collision leaves, every fifth a negative speed."""
    rng = np.random.default_rng(1000 + seed)
    d = np.stack([rng.uniform(-0.4189, 0.4189, M), rng.uniform(0.0, 20.0, M), rng.uniform(-6.0, 6.0, M),
                  rng.uniform(-0.6, 0.6, M)], axis=1)
    d[3::4] = 0.0
    d[4::5, 1] = -rng.uniform(0.1, 5.0, len(d[4::5]))
    return d


def states_from_poses(poses, n_envs, n_agents, seed=0):
    """A float64 state [7, E*A] whose cars take their (x, y, yaw) from `poses` [M, 3] (float32
    values) in a seeded order, and their other rows from dyn_columns."""
    rng = np.random.default_rng(seed + 7 * n_envs + n_agents)
    EA = n_envs * n_agents
    pick = rng.integers(0, len(poses), EA)
    dyn = dyn_columns(EA, seed)
    st = np.empty((7, EA))
    st[0], st[1], st[4] = (poses[pick, k].astype(np.float64) for k in range(3))
    st[2], st[3], st[5], st[6] = dyn.T
    return st


def state_of(cars):
    """A state [7, len(cars)] from rows (x, y, yaw[, v[, delta, yaw_rate, slip]])."""
    st = np.zeros((7, len(cars)))
    for c, row in enumerate(cars):
        row = list(row) + [0.0] * (7 - len(row))
        st[0, c], st[1, c], st[4, c], st[3, c], st[2, c], st[5, c], st[6, c] = row
    return st


def assert_rows_close(got, want, what=""):
    """The project's bar for float32 outputs of an f64 rule (pursuit_cases.assert_actions_close):
    one float32 ulp of the expected value or 1e-12 absolute."""
    C.assert_actions_close(got, want, what)


def assert_rows_equal(got, want, what=""):
    """Equal as float32 bits (NaN in both counts as equal only with the same bits)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), (what, np.argwhere(~same)[:5].tolist(), got[~same][:5], want[~same][:5])
