"""What tests/test_race_host.py and tests/test_gpu_race.py share: the tracks and call sequences the
race statistics are checked on, `NpRace` -- the rule of include/f110.h ("race statistics") in Python
floats over oracle/reward_oracle.py's TrackOracle.project_xy, with a plain Python tally of the
totals -- a runner of the host hook over the same buffers, and the comparisons.

Observations use n_beams = 4 (obs_len = 12) wherever no simulator is involved, so every case is
tiny."""
import math
import os

import numpy as np

from conftest import MAPS
from pursuit_cases import small_tracks, special_poses, track_poses  # noqa: F401 (special_poses: for the GPU tests)
from reward_oracle import TrackOracle

N_BEAMS = 4
OBS_LEN = N_BEAMS + 8
EGO, OPP = slice(N_BEAMS, N_BEAMS + 4), slice(N_BEAMS + 4, N_BEAMS + 8)
SQUARE = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 8.0], [0.0, 8.0], [0.0, 0.0]])  # L = 32, four segments
STARTED, CLOSED, S0, S1, AHEAD, OPP_CRASHED = 1, 2, 4, 8, 16, 32   # f110_race_state.flags
FINISHED, EGO_CRASH, COMPLETED, TRUNCATED, OPP_CRASH, AHEAD_AT_END = 1, 2, 4, 8, 16, 32  # the result byte
STATE = np.dtype([("s_prev", "<f8", 2), ("prog", "<f8", 2), ("lead0", "<f8"), ("t_max", "<f8"), ("len", "<i4"),
                  ("passes", "<i4"), ("passed", "<i4"), ("flags", "<i4")])
assert STATE.itemsize == 64
INT_TOTALS = ("episodes", "ego_crashes", "completed", "truncated", "opp_crashes", "ahead_at_end", "passes", "passed",
              "length_sum")


def race_tracks():
    """name -> (xy, closed): pursuit_cases.small_tracks(), Spielberg, and a closed 8 m square whose
    arclengths along the edges are exact in f64."""
    with np.load(os.path.join(MAPS, "Spielberg_centerline.npz")) as z:
        spielberg = z["xy"].copy()
    return {**small_tracks(), "spielberg": (spielberg, True), "square": (SQUARE, True)}


def make_track(name, device=None):
    """(reward.CenterlineTrack, TrackOracle) of race_tracks()[name]; device None: host arrays only."""
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    xy, closed = race_tracks()[name]
    return CenterlineTrack(xy, closed=closed, device=device), TrackOracle(xy, closed=closed)


def point_at(T, s):
    """The centerline point at arclength s of TrackOracle T (exact on the square's edges)."""
    i = T.seg_at(s)
    return T.xy[i] + (s - T.s[i]) * T.tan[i]


def obs_rows(ego_xy, opp_xy=None, col0=0.0, col1=0.0):
    """float32 obs [n, OBS_LEN] with the given points as the two pose groups (yaw 0)."""
    ego_xy = np.atleast_2d(np.asarray(ego_xy, np.float64))
    n = len(ego_xy)
    o = np.zeros((n, OBS_LEN), np.float32)
    o[:, :N_BEAMS] = 0.5
    o[:, N_BEAMS:N_BEAMS + 2] = ego_xy
    o[:, N_BEAMS + 3] = col0
    if opp_xy is not None:
        o[:, N_BEAMS + 4:N_BEAMS + 6] = np.atleast_2d(np.asarray(opp_xy, np.float64))
        o[:, N_BEAMS + 7] = col1
    return o


def flags(n, term=0, trunc=0, wr=0):
    return tuple(np.broadcast_to(np.asarray(v, np.uint8), (n,)).copy() for v in (term, trunc, wr))


def random_walk(T, n, calls=40, seed=0, p_bad=0.02, extra_poses=None):
    """`calls` rows of (obs [n, OBS_LEN] float32, terminated, truncated, was_reset): both cars start
    on pursuit_cases.track_poses (plus extra_poses) and move by small random steps; now and then a
    car's x or y is NaN / Inf for a row; collision entries and flags are drawn as
    test_episode_stats_kernel_matches_host draws its flags (rows with both flags set, resets rare
    enough that closed envs step on)."""
    rng = np.random.default_rng(seed + 17 * n)
    base = track_poses(T)[:, :2].astype(np.float64)
    if extra_poses is not None:
        base = np.concatenate([base, np.asarray(extra_poses, np.float64)[:, :2]])
    M = len(base)
    pos = np.stack([base[(3 * np.arange(n)) % M], base[(5 * np.arange(n) + 1) % M]], axis=1)  # [n, 2 cars, 2]
    out = []
    for _ in range(calls):
        wr = (rng.random(n) < 0.05).astype(np.uint8)
        jump = rng.integers(0, M, (n, 2))
        pos = np.where(wr[:, None, None] != 0, base[jump], pos + rng.normal(0.0, 0.3, (n, 2, 2)))
        pos = np.where(np.isfinite(pos), pos, base[jump])  # (a non-finite base pose does not stick)
        p = pos.copy()
        bad = rng.random((n, 2)) < p_bad
        kind = rng.integers(0, 3, (n, 2))
        p[..., 0] = np.where(bad & (kind == 0), np.nan, p[..., 0])
        p[..., 1] = np.where(bad & (kind == 1), np.inf, p[..., 1])
        p[..., 0] = np.where(bad & (kind == 2), -np.inf, p[..., 0])
        o = np.zeros((n, OBS_LEN), np.float32)
        o[:, :N_BEAMS] = rng.random((n, N_BEAMS))
        o[:, N_BEAMS:N_BEAMS + 2] = p[:, 0]
        o[:, N_BEAMS + 4:N_BEAMS + 6] = p[:, 1]
        o[:, N_BEAMS + 2] = o[:, N_BEAMS + 6] = rng.uniform(-3.0, 3.0, n)
        o[:, N_BEAMS + 3] = rng.random(n) < 0.1
        o[:, N_BEAMS + 7] = rng.random(n) < 0.1
        term = (rng.random(n) < 0.08).astype(np.uint8)
        trunc = (rng.random(n) < 0.08).astype(np.uint8)
        both = rng.random(n) < 0.02
        term[both] = trunc[both] = 1
        out.append((o, term, trunc, wr))
    return out


class Buffers:
    """The per-env arrays and totals one instance of the statistics owns, on the host."""

    def __init__(self, n):
        self.n = n
        self.state = np.zeros(n, STATE)
        self.cur = np.zeros((n, 2))
        self.last_progress, self.last_lead = np.zeros(n), np.zeros(n)
        self.last_length = np.zeros(n, np.int32)
        self.result = np.zeros(n, np.uint8)


class NpRace(Buffers):
    """The rule in Python floats, one env at a time, and a plain tally of what finished."""

    def __init__(self, T, n, has_opp=True, pass_margin=0.58, direction=1):
        super().__init__(n)
        self.T, self.has_opp, self.margin, self.dir = T, has_opp, float(pass_margin), float(direction)
        self.tally = dict.fromkeys(INT_TOTALS, 0)
        self.progress, self.leads, self.t_max = [], [], 0.0  # every finished episode's

    def wrap(self, d):
        if self.T.closed:
            if d > self.T.L / 2:
                d -= self.T.L
            if d < -self.T.L / 2:
                d += self.T.L
        return d

    def lead(self, st):
        return float(st["lead0"] + (st["prog"][0] - st["prog"][1])) if self.has_opp else 0.0

    def update(self, obs, term, trunc, wr):
        for e in range(self.n):
            self.result[e] = self.row(e, obs[e], int(term[e]), 0 if trunc is None else int(trunc[e]), int(wr[e]))
            self.cur[e] = (self.state[e]["prog"][0], self.lead(self.state[e]))

    def row(self, e, o, term, trunc, wr):
        st = self.state[e]
        groups = [o[EGO], o[OPP]] if self.has_opp else [o[EGO]]
        s, t, ok = [0.0, 0.0], [0.0, 0.0], [False, False]
        for k, g in enumerate(groups):
            x, y = float(g[0]), float(g[1])
            if math.isfinite(x) and math.isfinite(y):
                s[k], t[k] = self.T.project_xy(x, y)
                ok[k] = True
        col = [float(g[3]) != 0.0 for g in groups] + [False]
        if wr or not st["flags"] & STARTED:                         # 1. start row
            self.state[e] = np.zeros((), STATE)
            st = self.state[e]
            fl = STARTED
            for k in range(2):
                if ok[k]:
                    st["s_prev"][k] = s[k]
                    fl |= S0 << k
            lead0 = self.wrap(self.dir * (s[0] - s[1])) if ok[0] and ok[1] else 0.0
            st["lead0"] = lead0
            st["flags"] = fl | (AHEAD if lead0 > 0.0 else 0)
            return 0
        if st["flags"] & CLOSED:                                     # 2. closed row
            return 0
        fl = int(st["flags"])
        for k in range(2):                                           # 3. progress
            if ok[k]:
                if fl & (S0 << k):
                    st["prog"][k] = float(st["prog"][k]) + self.dir * self.wrap(s[k] - float(st["s_prev"][k]))
                st["s_prev"][k] = s[k]
                fl |= S0 << k
        st["len"] += 1
        if ok[0]:
            st["t_max"] = max(float(st["t_max"]), abs(t[0]))
        lead = 0.0
        if self.has_opp:                                             # 4. lead and passes
            if col[1]:
                fl |= OPP_CRASHED
            lead = self.lead(st)
            if not fl & AHEAD and lead > self.margin:
                fl |= AHEAD
                st["passes"] += 1
            elif fl & AHEAD and lead < -self.margin:
                fl &= ~AHEAD
                st["passed"] += 1
        st["flags"] = fl
        if not (term or trunc):                                      # 6.
            return 0
        st["flags"] = fl | CLOSED                                    # 5. finish
        res = FINISHED
        if term:
            res |= EGO_CRASH if col[0] else COMPLETED
        else:
            res |= TRUNCATED
        if fl & OPP_CRASHED:
            res |= OPP_CRASH
        if self.has_opp and lead > 0.0:
            res |= AHEAD_AT_END
        self.last_progress[e], self.last_lead[e], self.last_length[e] = st["prog"][0], lead, st["len"]
        ty = self.tally
        ty["episodes"] += 1
        ty["ego_crashes"] += bool(res & EGO_CRASH)
        ty["completed"] += bool(res & COMPLETED)
        ty["truncated"] += bool(res & TRUNCATED)
        ty["opp_crashes"] += bool(res & OPP_CRASH)
        ty["ahead_at_end"] += bool(res & AHEAD_AT_END)
        ty["passes"] += int(st["passes"])
        ty["passed"] += int(st["passed"])
        ty["length_sum"] += int(st["len"])
        self.progress.append(float(st["prog"][0]))
        self.leads.append(lead)
        self.t_max = max(self.t_max, float(st["t_max"]))
        return res

    def totals(self):
        """The tally as RaceStats.totals() reports it (sums by math.fsum) and the bound's two Σ|summand|."""
        t = dict(self.tally)
        n = t["episodes"]
        t.update(progress_sum=math.fsum(self.progress), lead_sum=math.fsum(self.leads), t_max=self.t_max,
                 progress_min=min(self.progress) if n else None, progress_max=max(self.progress) if n else None)
        return t, {"progress_sum": math.fsum(map(abs, self.progress)), "lead_sum": math.fsum(map(abs, self.leads))}


class HostRace(Buffers):
    """f110_host_race_stats on its own host buffers (any of the optional outputs may be dropped)."""

    def __init__(self, track, n, has_opp=True, pass_margin=None, direction=1, optional=True):
        from f110_gymnasium_ros2_jazzy_amd import _lib
        from f110_gymnasium_ros2_jazzy_amd.race import race_params
        super().__init__(n)
        self.track, self.has_opp, self.optional = track, has_opp, optional
        self.params = race_params(pass_margin, direction)
        self.c_totals = _lib.F110RaceTotals()
        self.abs_sums = {"progress_sum": 0.0, "lead_sum": 0.0}  # Σ|summand| of the two f64 sums

    def update(self, obs, term, trunc, wr):
        from f110_gymnasium_ros2_jazzy_amd.race import host_race_stats
        opt = (self.cur, self.last_progress, self.last_lead, self.last_length) if self.optional else (None,) * 4
        host_race_stats(self.track, self.params, obs[:, EGO], obs[:, OPP] if self.has_opp else None, term, trunc, wr,
                        self.state.view(np.uint8).reshape(self.n, 64), *opt, self.result, self.c_totals)
        fin = (self.result & FINISHED) != 0
        lead = self.state["lead0"] + (self.state["prog"][:, 0] - self.state["prog"][:, 1]) if self.has_opp else \
            np.zeros(self.n)
        self.abs_sums["progress_sum"] += float(np.abs(self.state["prog"][fin, 0]).sum())
        self.abs_sums["lead_sum"] += float(np.abs(lead[fin]).sum())

    def totals(self):
        from f110_gymnasium_ros2_jazzy_amd.race import totals_dict
        return totals_dict(self.c_totals), self.abs_sums


def assert_rows_equal(got, want, what="", optional=True):
    """Bit for bit per env: state, result and (optional) cur and the last_* arrays.  got / want:
    Buffers, or anything with the same attributes as NumPy arrays."""
    gs, ws = np.asarray(got.state).view(np.uint8).reshape(-1, 64), np.asarray(want.state).view(np.uint8).reshape(-1, 64)
    bad = np.flatnonzero((gs != ws).any(axis=1))
    assert bad.size == 0, (what, "state", bad[:5].tolist(), gs[bad[:2]].view(STATE), ws[bad[:2]].view(STATE))
    assert np.array_equal(got.result, want.result), (what, "result", got.result, want.result)
    if optional:
        for k in ("cur", "last_progress", "last_lead"):
            g, w = np.asarray(getattr(got, k), np.float64), np.asarray(getattr(want, k), np.float64)
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, k, g, w)
        assert np.array_equal(got.last_length, want.last_length), (what, "last_length")


def assert_totals_match(got, want, abs_sums, what=""):
    """Integer totals, min / max and t_max equal; the f64 sums within 1e-12 x the sum of |summand|
    (the bound of the episode-statistics test: the two sides add the same numbers in another
    order)."""
    for k in INT_TOTALS + ("progress_min", "progress_max", "t_max"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("progress_sum", "lead_sum"):
        print(f"{what}: {k} difference {got[k] - want[k]:+.3e}, bound {1e-12 * abs_sums[k]:.3e}")
        assert abs(got[k] - want[k]) <= 1e-12 * abs_sums[k], (what, k, got[k], want[k])
