"""Race statistics on the device: f110_race_stats (k_race_project, k_race, k_race_finish) against
its host statement on the tracks and walks of test_race_host.py, the projection's corner cases, row
ranges of a larger buffer, a captured update, F110VectorEnv's infos["race"] and race_totals() step by
step against the hook, and VectorTrainer's two row ranges inside the step graphs."""
import ctypes

import numpy as np
import pytest
import torch

import pursuit_cases as C
import race_cases as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 65, 257)  # one half-wave pair, a block of four envs, an odd tail, several blocks, a second reduction block


@pytest.fixture(scope="module")
def cases(gpu):
    """name -> (device CenterlineTrack, TrackOracle); built once."""
    out = {name: R.make_track(name, device=0) for name in R.race_tracks()}
    yield out
    for tr, _ in out.values():
        tr.close()


class DevView:
    """A RaceStats' buffers as the NumPy arrays race_cases compares."""

    def __init__(self, rs):
        self.state = rs.state.cpu().numpy()
        self.result = rs.result.cpu().numpy()
        self.cur = np.stack([rs.progress.cpu().numpy(), rs.lead.cpu().numpy()], axis=1)
        self.last_progress, self.last_lead = rs.last_progress.cpu().numpy(), rs.last_lead.cpu().numpy()
        self.last_length = rs.last_length.cpu().numpy()


def _stats(gpu, track, n, has_opp=True, **kw):
    from f110_gymnasium_ros2_jazzy_amd.race import RaceStats
    return RaceStats(n, track, R.N_BEAMS, opponent_idx=1 if has_opp else None, device=gpu, **kw)


def _dev(gpu, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _totals_bytes(rs):
    return rs._totals.cpu().numpy().tobytes()


class RawRace:
    """f110_race_stats called directly, with every optional argument NULL."""

    def __init__(self, gpu, track, n):
        from f110_gymnasium_ros2_jazzy_amd import _lib
        from f110_gymnasium_ros2_jazzy_amd.race import race_params
        self.F, self.L, self.gpu, self.track, self.n = _lib, _lib.load(), gpu, track, n
        self.params = race_params()
        self.state = torch.zeros(n, 64, dtype=torch.uint8, device=gpu)
        self.result = torch.zeros(n, dtype=torch.uint8, device=gpu)
        self.totals = torch.zeros(112, dtype=torch.uint8, device=gpu)
        self.scratch = torch.zeros(int(self.L.f110_race_scratch_bytes(n)), dtype=torch.uint8, device=gpu)

    def update(self, obs, term, wr):
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        o, te, w = _dev(self.gpu, obs, term, wr)
        ego = ctypes.c_void_p(o.data_ptr() + 4 * R.N_BEAMS)
        s = ctypes.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream)
        self.F.check(self.L.f110_race_stats(self.track.handle, ctypes.byref(self.params), ego, None, R.OBS_LEN, P(te),
                                            None, P(w), self.n, P(self.state), None, None, None, None, P(self.result),
                                            P(self.totals), P(self.scratch), s), "f110_race_stats")


# ---- 1. the kernels against the host hook ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.race_tracks()))
@pytest.mark.parametrize("n", NS)
def test_kernel_matches_host(gpu, cases, name, n):
    from f110_gymnasium_ros2_jazzy_amd.race import totals_dict
    track, T = cases[name]
    walk = R.random_walk(T, n, calls=40, seed=3)
    dev = [_stats(gpu, track, n) for _ in range(2)]
    host = R.HostRace(track, n)
    for i, (obs, term, trunc, wr) in enumerate(walk):
        host.update(obs, term, trunc, wr)
        for d in dev:
            d.update(*_dev(gpu, obs, term, trunc, wr))
        R.assert_rows_equal(DevView(dev[0]), host, f"{name} n={n} call {i}")
    want, abs_sums = host.totals()
    R.assert_totals_match(dev[0].totals(), want, abs_sums, f"{name} n={n}")
    assert _totals_bytes(dev[0]) == _totals_bytes(dev[1]) and dev[0].totals() == dev[1].totals()
    if n >= 65:
        assert want["episodes"] > 0 and want["truncated"] > 0 and want["ego_crashes"] + want["completed"] > 0
    # truncated = NULL; opp = NULL; every optional output NULL (also without truncated and opponent)
    variants = [(_stats(gpu, track, n), R.HostRace(track, n), False, True),
                (_stats(gpu, track, n, has_opp=False), R.HostRace(track, n, has_opp=False), True, False)]
    raw, raw_host = RawRace(gpu, track, n), R.HostRace(track, n, has_opp=False, optional=False)
    for i, (obs, term, trunc, wr) in enumerate(walk[:15]):
        for d, h, use_trunc, _ in variants:
            tr = trunc if use_trunc else None
            h.update(obs, term, tr, wr)
            d.update(*_dev(gpu, obs, term, tr, wr))
            R.assert_rows_equal(DevView(d), h, f"{name} n={n} variant call {i}")
        raw.update(obs, term, wr)
        raw_host.update(obs, term, None, wr)
        assert np.array_equal(raw.state.cpu().numpy(), raw_host.state.view(np.uint8).reshape(n, 64)), i
        assert np.array_equal(raw.result.cpu().numpy(), raw_host.result), i
    for d, h, _, has_opp in variants:
        R.assert_totals_match(d.totals(), *h.totals(), f"{name} n={n} variant")
        if not has_opp:
            assert not bool(d.lead.any()) and not bool((d.result & R.AHEAD_AT_END).any())
    got = totals_dict(raw.F.F110RaceTotals.from_buffer_copy(raw.totals.cpu().numpy().tobytes()))
    R.assert_totals_match(got, *raw_host.totals(), f"{name} n={n} raw")


# ---- 2. the projection's corner cases ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.race_tracks()))
def test_projection_corner_cases(gpu, cases, name):
    """track_poses and special_poses rows (off the grid, ties, node hits, clusters, non-finite
    entries) as the ego's and the opponent's poses, in three different pairings."""
    track, T = cases[name]
    poses = np.concatenate([C.track_poses(T, spread=3.0 if name == "spielberg" else 1.5), C.special_poses()])
    n = len(poses)
    dev, host = _stats(gpu, track, n), R.HostRace(track, n)
    for i, shift in enumerate((7, 1, n // 2)):
        obs = np.zeros((n, R.OBS_LEN), np.float32)
        obs[:, R.N_BEAMS:R.N_BEAMS + 3] = np.roll(poses, i, axis=0)
        obs[:, R.N_BEAMS + 4:R.N_BEAMS + 7] = np.roll(poses, shift, axis=0)
        fl = R.flags(n, wr=i == 0, trunc=i == 2)
        host.update(obs, *fl)
        dev.update(*_dev(gpu, obs, *fl))
        R.assert_rows_equal(DevView(dev), host, f"{name} pairing {i}")
    R.assert_totals_match(dev.totals(), *host.totals(), name)
    assert host.totals()[0]["episodes"] == n


# ---- 3. row ranges of a larger buffer ----------------------------------------------------------------
def test_row_ranges(gpu, cases):
    track, T = cases["spielberg"]
    n, k = 65, 7
    full, part = _stats(gpu, track, n), _stats(gpu, track, n - k)
    for obs, term, trunc, wr in R.random_walk(T, n, calls=25, seed=9):
        o, te, tr, w = _dev(gpu, obs, term, trunc, wr)
        full.update(o, te, tr, w)
        part.update(o[k:], te[k:], tr[k:], w[k:])
        a, b = DevView(full), DevView(part)
        for f in ("state", "result", "cur", "last_progress", "last_lead", "last_length"):
            assert getattr(a, f)[k:].tobytes() == getattr(b, f).tobytes(), f
    assert part.totals()["episodes"] > 0


# ---- 4. graph capture ----------------------------------------------------------------------------------
def test_update_is_capturable(gpu, cases):
    track, T = cases["triangle"]
    n = 65
    walk = R.random_walk(T, n, calls=6, seed=4)
    eager, graphed = _stats(gpu, track, n), _stats(gpu, track, n)
    bufs = _dev(gpu, *walk[0])
    for rs in (eager, graphed):
        rs.begin(bufs[0])
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.update(*bufs)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for call in walk[1:]:
        new = _dev(gpu, *call)
        for b, v in zip(bufs, new):
            b.copy_(v)
        g.replay()
        eager.update(*new)
    torch.cuda.synchronize()
    assert torch.equal(eager.state, graphed.state) and torch.equal(eager.result, graphed.result)
    assert _totals_bytes(eager) == _totals_bytes(graphed)
    assert eager.totals()["episodes"] > 0


# ---- 5. F110VectorEnv ------------------------------------------------------------------------------------
B = 1080


def test_vector_env_race_infos(gpu, cases):
    from f110_gymnasium_ros2_jazzy_amd import opponent as O
    from f110_gymnasium_ros2_jazzy_amd.race import host_race_stats, race_params
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    track, T = cases["spielberg"]
    n, steps = 70, 150
    env = F110VectorEnv(n, num_agents=2, seed=7, device=gpu, noise_std=0.0, opponent="pure_pursuit",
                        opponent_track=track, opponent_speed=2.0, max_episode_steps=60, episode_stats=True,
                        race_stats=True)
    try:
        obs, infos = env.reset(options=C.lap_spawns(T, n, lead=-20).astype(np.float32))
        rec = [(obs.cpu().numpy(), np.zeros(n, np.uint8), None, np.ones(n, np.uint8), infos["race"])]
        for _ in range(steps):
            ego = O.pure_pursuit(obs[:, B:B + 4], track, speed=7.0)
            obs, _, term, trunc, infos = env.step(ego)
            assert torch.equal(infos["race"]["finished"], infos["episode"]["finished"])
            rec.append((obs.cpu().numpy(), term.cpu().numpy().astype(np.uint8), trunc.cpu().numpy().astype(np.uint8),
                        infos["reset"].cpu().numpy().astype(np.uint8), infos["race"]))
        got = env.race_totals()
        # the host hook over the recorded observations and flags
        from f110_gymnasium_ros2_jazzy_amd import _lib
        h = R.Buffers(n)
        totals, abs_sums = _lib.F110RaceTotals(), {"progress_sum": 0.0, "lead_sum": 0.0}
        for i, (o, te, tr, wr, race) in enumerate(rec):
            host_race_stats(track, race_params(), o[:, B:B + 4], o[:, B + 4:B + 8], te, tr, wr,
                            h.state.view(np.uint8).reshape(n, 64), h.cur, h.last_progress, h.last_lead, h.last_length,
                            h.result, totals)
            assert np.array_equal(race["result"].cpu().numpy(), h.result), i
            for k, col in (("progress", 0), ("lead", 1)):
                assert np.array_equal(race[k].cpu().numpy().view(np.uint64), h.cur[:, col].view(np.uint64)), (i, k)
            assert np.array_equal(race["finished"].cpu().numpy(), (h.result & 1) != 0), i
            fin = (h.result & 1) != 0
            abs_sums["progress_sum"] += float(np.abs(h.cur[fin, 0]).sum())
            abs_sums["lead_sum"] += float(np.abs(h.cur[fin, 1]).sum())
        from f110_gymnasium_ros2_jazzy_amd.race import totals_dict
        want = totals_dict(totals)
        print({k: want[k] for k in R.INT_TOTALS}, want["progress_mean"], want["lead_mean"])
        R.assert_totals_match(got, want, abs_sums, "env")
        assert want["episodes"] >= n and want["truncated"] > 0 and want["progress_sum"] > 0.0
        env.reset_race_totals()
        assert env.race_totals()["episodes"] == 0 and env.race_totals()["progress_mean"] is None
    finally:
        env.close()


def test_vector_env_defaults_are_unchanged(gpu, cases):
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    env = F110VectorEnv(4, num_agents=2, seed=7, device=gpu, opponent="gap_follow")
    try:
        _, infos = env.reset(seed=1)
        keys = {"poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions", "lap_times",
                "lap_counts", "scans", "time", "reset", "opponent_actions"}
        assert set(infos) == keys
        _, _, _, _, infos = env.step(torch.zeros(4, 2, device=gpu))
        assert set(infos) == keys
        with pytest.raises(ValueError, match="race_stats=True"):
            env.race_totals()
        with pytest.raises(ValueError, match="race_stats=True"):
            env.reset_race_totals()
    finally:
        env.close()
    with pytest.raises(ValueError, match="needs a centerline"):
        F110VectorEnv(4, num_agents=2, seed=7, device=gpu, opponent="gap_follow", race_stats=True)
    # a single-agent env has no opponent part; infos="minimal" carries the key too
    track = cases["spielberg"][0]
    env = F110VectorEnv(4, num_agents=1, seed=7, device=gpu, race_stats=True, race_track=track, infos="minimal",
                        max_episode_steps=5)
    try:
        env.reset(seed=1)
        for _ in range(6):
            _, _, _, _, infos = env.step(torch.tensor([[0.0, 2.0]] * 4, device=gpu))
        assert set(infos) == {"reset", "truncation", "race"} and not bool(infos["race"]["lead"].any())
        t = env.race_totals()
        assert t["episodes"] == 4 and t["truncated"] == 4 and t["ahead_at_end"] == 0 and t["lead_sum"] == 0.0
    finally:
        env.close()


# ---- 6. the trainer ----------------------------------------------------------------------------------------
def test_trainer_race_stats_in_step_graphs(gpu):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer, episode_report
    tr = VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=8, graphs=True, max_episode_steps=20,
                       eval_envs=8, race_stats=True)
    try:
        for _ in range(80):
            tr.step()
        assert (0, True) in tr._sg and (1, True) in tr._sg  # the graphed path was reached, both parities
        for race, ep in ((tr.train_race, tr.train_stats), (tr.eval_race, tr.eval_stats)):
            r, e = race.totals(), ep.totals()
            assert r["episodes"] == e["episodes"] > 0 and r["length_sum"] == e["length_sum"]
            assert r["truncated"] == e["truncated"] and r["ego_crashes"] + r["completed"] == e["terminated"]
        want = tr.train_race.totals()
        rep = episode_report(tr)
        for prefix in ("", "eval_"):
            for k in ("race_episodes", "progress_mean", "lead_mean", "win_rate", "crash_rate", "passes_per_episode"):
                assert rep[prefix + k] is not None, prefix + k
        assert rep["race_episodes"] == rep["episodes"] == want["episodes"]
        assert rep["progress_mean"] == want["progress_sum"] / want["episodes"] and rep["win_rate"] == want["win_rate"]
        assert tr.train_race.totals()["episodes"] == 0 and tr.eval_race.totals()["episodes"] == 0
    finally:
        tr.close()
    tr = VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=8, graphs=True, max_episode_steps=20,
                       eval_envs=8)
    try:
        for _ in range(24):
            tr.step()
        rep = episode_report(tr)
        assert not any("race" in k or "progress" in k or "win_rate" in k for k in rep), rep
        assert tr.train_race is None and tr.env._race is None
    finally:
        tr.close()
