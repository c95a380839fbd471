"""Race statistics, host side (no GPU): the new entry points are exported under ABI 3 with the
declared struct sizes, f110_host_race_stats -- the device's row rule and totals merge over host
arrays -- follows race_cases.NpRace bit for bit on random walks over every track, gives the known
answers on the 8 m square and the open track, counts passes and outcomes as include/f110.h states
them, and both entry points refuse what they must."""
import ctypes

import numpy as np
import pytest

import race_cases as R


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def square():
    return R.make_track("square")


def test_exports_sizes_and_abi(F):
    L = F.load()
    for n in ("f110_default_race_params", "f110_race_scratch_bytes", "f110_race_stats", "f110_host_race_stats"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION
    assert ctypes.sizeof(F.F110RaceParams) == 16
    assert ctypes.sizeof(F.F110RaceState) == 64 == F.RACE_STATE_BYTES == R.STATE.itemsize
    assert ctypes.sizeof(F.F110RaceTotals) == 112 == F.RACE_TOTALS_BYTES
    for f in R.STATE.names:
        assert getattr(F.F110RaceState, f).offset == R.STATE.fields[f][1], f
    p = F.F110RaceParams()
    L.f110_default_race_params(ctypes.byref(p))
    assert (p.pass_margin, p.direction) == (0.58, 1)
    assert L.f110_race_scratch_bytes(1) > 0 and L.f110_race_scratch_bytes(1000) > L.f110_race_scratch_bytes(1)


# ---- the hook against the Python statement of the rule ------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.race_tracks()))
@pytest.mark.parametrize("has_opp,direction", [(True, 1), (True, -1), (False, 1)])
def test_host_race_stats_matches_np_race(F, name, has_opp, direction):
    track, T = R.make_track(name)
    n = 6
    walk = R.random_walk(T, n, calls=40, seed=direction + 2 * has_opp)
    host = R.HostRace(track, n, has_opp=has_opp, direction=direction)
    model = R.NpRace(T, n, has_opp=has_opp, direction=direction)
    seen = set()
    for i, (obs, term, trunc, wr) in enumerate(walk):
        closed_before = (model.state["flags"] & R.CLOSED) != 0
        host.update(obs, term, trunc, wr)
        model.update(obs, term, trunc, wr)
        R.assert_rows_equal(host, model, f"{name} call {i}")
        seen |= {"closed_step"} if np.any(closed_before & (wr == 0)) else set()
        seen |= {"bad_pose"} if not np.isfinite(obs).all() else set()
    want, abs_model = model.totals()
    got, abs_host = host.totals()
    assert abs_host == pytest.approx(abs_model)
    R.assert_totals_match(got, want, abs_model, name)
    assert want["episodes"] > 0 and want["truncated"] > 0 and want["ego_crashes"] + want["completed"] > 0
    assert {"closed_step", "bad_pose"} <= seen
    if not has_opp:
        assert got["passes"] == got["passed"] == got["ahead_at_end"] == got["opp_crashes"] == 0 and got["lead_sum"] == 0.0
    track.close()


def test_optional_outputs_may_be_null(F):
    track, T = R.make_track("triangle")
    n = 5
    full, bare = R.HostRace(track, n), R.HostRace(track, n, optional=False)
    zeros, null = R.HostRace(track, n), R.HostRace(track, n)
    for i, (obs, term, trunc, wr) in enumerate(R.random_walk(T, n, calls=20, seed=5)):
        full.update(obs, term, trunc, wr)
        bare.update(obs, term, trunc, wr)
        R.assert_rows_equal(bare, full, f"call {i}", optional=False)
        zeros.update(obs, term, np.zeros_like(trunc), wr)
        null.update(obs, term, None, wr)          # NULL truncated: as all zeros
        R.assert_rows_equal(null, zeros, f"call {i}")
    assert not bare.cur.any() and not bare.last_length.any() and not bare.last_progress.any()
    assert bare.totals()[0] == full.totals()[0] and null.totals()[0] == zeros.totals()[0]
    assert full.totals()[0]["truncated"] > 0 == null.totals()[0]["truncated"]
    track.close()


# ---- known answers ----------------------------------------------------------------------------------
def _drive(track, ego_s, T, opp_s=None, direction=1, pass_margin=None, finish="trunc"):
    """One env: the ego (and the opponent) at the given arclengths, row by row; the last row ends the
    episode.  Returns the HostRace and the passes / passed counts after every row."""
    h = R.HostRace(track, 1, has_opp=opp_s is not None, direction=direction, pass_margin=pass_margin)
    counts = []
    for i, s in enumerate(ego_s):
        last = i == len(ego_s) - 1
        obs = R.obs_rows(R.point_at(T, s), None if opp_s is None else R.point_at(T, opp_s[i]))
        h.update(obs, *R.flags(1, term=last and finish == "term", trunc=last and finish == "trunc"))
        counts.append((int(h.state["passes"][0]), int(h.state["passed"][0])))
    return h, counts


@pytest.mark.parametrize("direction", [1, -1])
def test_square_laps_are_exact(square, direction):
    track, T = square
    assert T.L == 32.0
    fwd = [float(k % 32) for k in range(33)]          # 0, 1, .. 31, 0: crosses s = L -> 0 once
    h, _ = _drive(track, fwd, T, direction=direction)
    assert h.last_progress[0] == 32.0 * direction and h.cur[0, 0] == 32.0 * direction
    assert h.last_length[0] == 32 and h.result[0] == R.FINISHED | R.TRUNCATED
    h, _ = _drive(track, fwd[::-1], T, direction=direction)
    assert h.last_progress[0] == -32.0 * direction
    t, _ = h.totals()
    assert (t["episodes"], t["progress_sum"], t["progress_min"], t["progress_max"], t["length_sum"]) == \
        (1, -32.0 * direction, -32.0 * direction, -32.0 * direction, 32)
    assert t["lead_sum"] == 0.0 and t["t_max"] == 0.0


def test_open_track_does_not_wrap():
    track, T = R.make_track("open4")
    assert not T.closed
    # out and back on the first segment, then a jump of more than L / 2 to the last one
    h, _ = _drive(track, [0.0, 1.0, 2.0, 3.0, 4.0, 3.0, 2.0, 1.0], T)
    assert h.last_progress[0] == 1.0
    far = float(T.s[2]) + 3.5
    assert far - 0.5 > T.L / 2
    h, _ = _drive(track, [0.5, far], T)
    assert h.last_progress[0] == far - 0.5
    track.close()


def test_passes_are_counted_once_past_the_margin(square):
    track, T = square
    ego = [float(k) for k in range(13)]              # 1 m per row from 3 m behind
    opp = [3.0 + 0.5 * k for k in range(13)]         # 0.5 m per row: lead = -3 + k/2
    h, counts = _drive(track, ego, T, opp)
    first = next(k for k in range(13) if -3.0 + 0.5 * k > 0.58)
    assert first == 8
    assert counts == [(0, 0)] * first + [(1, 0)] * (13 - first)
    assert h.last_lead[0] == 3.0 and h.result[0] & R.AHEAD_AT_END
    t, _ = h.totals()
    assert (t["passes"], t["passed"], t["ahead_at_end"], t["lead_sum"]) == (1, 0, 1, 3.0)
    # mirrored: the ego is the slow car, 3 m ahead
    h, counts = _drive(track, opp, T, ego)
    assert counts == [(0, 0)] * first + [(0, 1)] * (13 - first)
    assert h.last_lead[0] == -3.0 and not h.result[0] & R.AHEAD_AT_END
    t, _ = h.totals()
    assert (t["passes"], t["passed"], t["ahead_at_end"], t["win_rate"]) == (0, 1, 0, 0.0)


def test_dead_band_and_zero_margin(square):
    track, T = square
    wobble = [4.25 if k % 2 == 0 else 3.75 for k in range(12)]   # lead +-0.25 around a standing opponent
    h, counts = _drive(track, wobble, T, [4.0] * 12)
    assert counts[-1] == (0, 0) and h.state["flags"][0] & R.AHEAD   # ahead from the start row, never passed
    h, counts = _drive(track, wobble[1:], T, [4.0] * 11)
    assert counts[-1] == (0, 0) and not h.state["flags"][0] & R.AHEAD
    h, counts = _drive(track, wobble[1:], T, [4.0] * 11, pass_margin=0.0)
    assert counts[0] == (0, 0) and counts[1] == (1, 0) and counts[2] == (1, 1)  # at the first positive lead


def test_outcomes(square):
    track, T = square
    n = 4
    h = R.HostRace(track, n)
    ahead = np.array([True, True, False, False])
    ego0 = np.array([R.point_at(T, 5.0 if a else 2.0) for a in ahead])
    opp0 = np.array([R.point_at(T, 2.0 if a else 5.0) for a in ahead])
    h.update(R.obs_rows(ego0, opp0), *R.flags(n, wr=1))
    h.update(R.obs_rows(ego0, opp0, col1=[0, 0, 1, 0]), *R.flags(n))     # env 2's opponent crashes mid-episode
    assert not h.result.any()
    h.update(R.obs_rows(ego0, opp0, col0=[1, 0, 0, 0]), *R.flags(n, term=[1, 1, 0, 1], trunc=[0, 0, 1, 1]))
    assert h.result.tolist() == [R.FINISHED | R.EGO_CRASH | R.AHEAD_AT_END, R.FINISHED | R.COMPLETED | R.AHEAD_AT_END,
                                 R.FINISHED | R.TRUNCATED | R.OPP_CRASH, R.FINISHED | R.COMPLETED]
    assert h.last_lead.tolist() == [3.0, 3.0, -3.0, -3.0] and h.last_length.tolist() == [2] * n
    t, _ = h.totals()
    assert [t[k] for k in R.INT_TOTALS] == [4, 1, 2, 1, 1, 2, 0, 0, 8]
    assert (t["win_rate"], t["crash_rate"], t["lead_mean"], t["length_mean"]) == (0.5, 0.25, 0.0, 2.0)


def test_row_kinds(square):
    track, T = square
    h = R.HostRace(track, 2)
    at = lambda s0, s1: R.obs_rows([R.point_at(T, s0)] * 2, [R.point_at(T, s1)] * 2)  # noqa: E731
    # the first call on zero state is a start row whatever its flags; so is a reset row with terminated
    h.update(at(1.0, 0.0), *R.flags(2, term=1))
    assert not h.result.any() and h.totals()[0]["episodes"] == 0
    assert (h.state["flags"] == R.STARTED | R.S0 | R.S1 | R.AHEAD).all() and (h.state["lead0"] == 1.0).all()
    h.update(at(2.0, 0.0), *R.flags(2))
    h.update(at(7.0, 0.0), *R.flags(2, term=1, wr=1))
    assert not h.result.any() and h.totals()[0]["episodes"] == 0 and (h.state["len"] == 0).all()
    assert (h.state["lead0"] == 7.0).all() and not h.cur[:, 0].any()
    # autoreset off: rows after a finish are ignored until a reset row
    h.update(at(8.0, 0.0), *R.flags(2, trunc=[1, 0]))
    assert h.result.tolist() == [R.FINISHED | R.TRUNCATED | R.AHEAD_AT_END, 0]
    frozen = h.state[0].copy()
    h.update(at(9.0, 0.0), *R.flags(2, term=1))
    assert h.result.tolist() == [0, R.FINISHED | R.COMPLETED | R.AHEAD_AT_END]
    assert h.state[0] == frozen and h.cur[0].tolist() == [1.0, 8.0] and h.last_length.tolist() == [1, 2]
    h.update(at(3.0, 0.0), *R.flags(2, wr=[1, 0]))
    assert h.state["flags"][0] == R.STARTED | R.S0 | R.S1 | R.AHEAD and h.state["flags"][1] & R.CLOSED
    assert h.state["len"].tolist() == [0, 2] and h.totals()[0]["episodes"] == 2


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_pose_keeps_the_car_in_place(square, bad):
    track, T = square
    h = R.HostRace(track, 1)
    row = lambda s0, s1: R.obs_rows(R.point_at(T, s0), R.point_at(T, s1))  # noqa: E731
    h.update(row(1.0, 0.0), *R.flags(1, wr=1))
    h.update(row(2.0, 0.5), *R.flags(1))
    o = row(3.0, 1.0)
    o[0, R.N_BEAMS + 1] = bad                      # the ego's y
    h.update(o, *R.flags(1))
    assert h.state["s_prev"][0].tolist() == [2.0, 1.0] and h.state["prog"][0].tolist() == [1.0, 1.0]
    assert h.state["len"][0] == 2
    h.update(row(4.0, 1.5), *R.flags(1))           # steps from the old s_prev
    assert h.state["prog"][0].tolist() == [3.0, 1.5] and h.cur[0].tolist() == [3.0, 2.5]
    # a start row with a car that is not ok: no s_prev, no lead0; its first finite row only sets s_prev
    h = R.HostRace(track, 1)
    o = row(3.0, 1.0)
    o[0, R.N_BEAMS + 4] = bad                      # the opponent's x
    h.update(o, *R.flags(1))
    assert h.state["flags"][0] == R.STARTED | R.S0 and h.state["lead0"][0] == 0.0
    h.update(row(4.0, 1.0), *R.flags(1))
    assert h.state["flags"][0] & R.S1 and h.state["prog"][0].tolist() == [1.0, 0.0]


def test_without_an_opponent(square):
    track, T = square
    h, counts = _drive(track, [float(k) for k in range(6)], T)
    assert counts[-1] == (0, 0) and h.last_progress[0] == 5.0 and h.last_lead[0] == 0.0
    assert not h.cur[:, 1].any() and h.result[0] == R.FINISHED | R.TRUNCATED
    assert not h.state["flags"][0] & (R.S1 | R.AHEAD | R.OPP_CRASHED) and h.state["lead0"][0] == 0.0


# ---- argument errors -------------------------------------------------------------------------------
def _call(F, fn, tr, host, **over):
    """One call of f110_race_stats / f110_host_race_stats with valid host-side arguments (device
    entry: the pointers are never followed, the checks come first) and the given ones replaced."""
    n = 2
    bufs = dict(ego=np.zeros((n, 4), np.float32), opp=np.zeros((n, 4), np.float32), term=np.zeros(n, np.uint8),
                trunc=np.zeros(n, np.uint8), wr=np.ones(n, np.uint8), state=np.zeros((n, 64), np.uint8),
                cur=np.zeros((n, 2)), lp=np.zeros(n), ll=np.zeros(n), llen=np.zeros(n, np.int32),
                result=np.zeros(n, np.uint8), scratch=np.zeros(4096, np.uint8))
    a = dict(track=tr.handle, params=F.F110RaceParams(0.58, 1, 0), stride=4, n=n, totals=F.F110RaceTotals(),
             **{k: ctypes.c_void_p(v.ctypes.data) for k, v in bufs.items()})
    a.update(over)
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    args = [a["track"], ref(a["params"]), a["ego"], a["opp"], a["stride"], a["term"], a["trunc"], a["wr"], a["n"],
            a["state"], a["cur"], a["lp"], a["ll"], a["llen"], a["result"], ref(a["totals"])]
    if not host:
        args += [a["scratch"], None]
    return fn(*args), bufs


BAD = [dict(track=None), dict(params=None), dict(ego=None), dict(term=None), dict(wr=None), dict(state=None),
       dict(result=None), dict(totals=None), dict(stride=3), dict(n=-1)] + \
      [dict(params=p) for p in ((-0.1, 1), (float("nan"), 1), (0.58, 0), (0.58, 2), (0.58, -2))]


@pytest.mark.parametrize("host", [True, False])
def test_argument_errors(F, square, host):
    track, _ = square
    L = F.load()
    fn = L.f110_host_race_stats if host else L.f110_race_stats
    for over in BAD + ([] if host else [dict(scratch=None)]):
        if isinstance(over.get("params"), tuple):
            over = dict(params=F.F110RaceParams(over["params"][0], over["params"][1], 0))
        rc, bufs = _call(F, fn, track, host, **over)
        assert rc == -1, over
        assert (L.f110_last_error() or b"").decode().startswith(fn.__name__ + ": bad arguments"), over
        assert not bufs["state"].any() and not bufs["result"].any()
    # the host hook works on a host-only track; the device entry refuses one
    rc, bufs = _call(F, fn, track, host)
    assert rc == (0 if host else -1)
    if host:
        assert bufs["state"].any()                   # the start row was taken
        rc, _ = _call(F, fn, track, host, opp=None, trunc=None, cur=None, lp=None, ll=None, llen=None, n=0)
        assert rc == 0
    else:
        assert b"device track" in L.f110_last_error()
