"""The sensor randomization on the device: f110_sensor_apply (k_sensor) against its host statement,
bit for bit on the rows, the parameter rows and the counters, in place and into a disjoint buffer;
one captured apply; reset(mask); F110VectorEnv(sensor_ranges=...) beside a twin without it, with and
without the scan observation behind it; step_transition into obs_out; and train.py's flags."""
import itertools

import numpy as np
import pytest
import torch

import pursuit_cases as PC
import sensor_cases as C

pytestmark = pytest.mark.gpu

B = 1080


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def S():
    from f110_gymnasium_ros2_jazzy_amd import sensor
    return sensor


@pytest.fixture(scope="module")
def track(gpu):
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    xy, _, _ = PC.spielberg_xy()
    tr = CenterlineTrack(xy, closed=True, device=0)
    yield tr
    tr.close()


def assert_state(model, host, what):
    dev = model.arrays()
    for k in ("params", "episode", "step"):
        assert C.same_bits(dev[k].cpu().numpy(), host[k]), (what, k)


@pytest.mark.parametrize("B_", C.BEAMS)
def test_kernel_matches_host(gpu, S, B_):
    """N = 3 at env_offset 7, every parameter active, six applies with a reset flag for one env at
    the third; row_stride and out_stride above the width; out disjoint and out = rows."""
    for M, T in itertools.product(C.MIDS, C.TAILS):
        for in_place in (False, True):
            rng = np.random.default_rng(B_ * 10 + M + T)
            W = B_ + M + T
            kw = dict(range_max=C.RANGE_MAX, seed=C.SEED, env_offset=C.ENV_OFFSET)
            model = S.SensorModel(C.N_ENVS, B_, M, T, device=gpu, **kw, **C.active(B_))
            try:
                host = S.host_sensor_state(C.N_ENVS)
                store = torch.full((C.N_ENVS, W + 3), -7.0, device=gpu)
                other = torch.full((C.N_ENVS, W + 5), -9.0, device=gpu)
                dev_rows = store[:, :W]
                out = dev_rows if in_place else other[:, :W]
                for t in range(C.APPLIES):
                    rows = C.rows_for(rng, C.N_ENVS, B_, M, T)
                    dev_rows.copy_(torch.as_tensor(rows))
                    reset = None
                    if t == C.RESET_AT:
                        reset = np.zeros(C.N_ENVS, np.uint8)
                        reset[C.RESET_ENV] = 1
                    got = model.apply(dev_rows, None if reset is None else torch.as_tensor(reset, device=gpu), out=out)
                    want = S.host_sensor_apply(host, rows, B_, M, T, reset=reset, **kw, **C.active(B_))
                    assert got.data_ptr() == out.data_ptr()
                    assert C.same_bits(got.cpu().numpy(), want), (M, T, in_place, t, "rows")
                    assert_state(model, host, (M, T, in_place, t))
                    if not in_place:
                        assert C.same_bits(dev_rows.cpu().numpy(), rows)  # the clean rows are left alone
                assert host["episode"].tolist() == [0, 1, 0] and host["step"].tolist() == [5, 3, 5]
                assert bool((store[:, W:] == -7.0).all()) and bool((other[:, W:] == -9.0).all())  # the pads are kept
            finally:
                model.close()


def test_identity_mask_and_reset(gpu, S):
    """The identity returns the row; a masked-off env gets its clean row while its counters advance;
    reset(mask) restarts the masked counters only; bad arrays are refused."""
    rng = np.random.default_rng(2)
    N, B_, M, T = 6, 130, 8, 5
    rows = C.rows_for(rng, N, B_, M, T)
    rows[0, :4] = [0.0, 1.0, np.float32(1e-42), -0.0]
    dev = torch.as_tensor(rows, device=gpu)
    ident = S.SensorModel(N, B_, M, T, device=gpu)
    try:
        assert same_bits(ident.apply(dev), dev) and same_bits(ident.apply(dev), dev)
    finally:
        ident.close()
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    kw = dict(seed=11, env_offset=3)
    model = S.SensorModel(N, B_, M, T, mask=mask, device=gpu, **kw, **C.active(B_))
    try:
        host = S.host_sensor_state(N)
        for t in range(3):
            got = model.apply(dev)
            want = S.host_sensor_apply(host, rows, B_, M, T, mask=mask, **kw, **C.active(B_))
            assert C.same_bits(got.cpu().numpy(), want), t
            assert C.same_bits(want[mask == 0], rows[mask == 0]) and not C.same_bits(want[0], rows[0])
        assert_state(model, host, "masked")
        assert host["step"].tolist() == [2] * N
        sel = np.array([1, 1, 0, 0, 0, 0], np.uint8)
        model.reset(torch.as_tensor(sel, device=gpu))
        host["episode"][sel != 0], host["step"][sel != 0] = -1, 0
        assert_state(model, host, "reset(mask)")
        got = model.apply(dev, torch.as_tensor(np.array([0, 0, 0, 1, 0, 0], bool), device=gpu))
        want = S.host_sensor_apply(host, rows, B_, M, T, mask=mask, reset=np.array([0, 0, 0, 1, 0, 0], np.uint8), **kw,
                                   **C.active(B_))
        assert C.same_bits(got.cpu().numpy(), want)
        assert_state(model, host, "after reset(mask)")
        assert host["episode"].tolist() == [0, 0, 0, 1, 0, 0] and host["step"].tolist() == [0, 0, 3, 0, 3, 3]
        model.reset()
        host["episode"][:], host["step"][:] = -1, 0
        assert_state(model, host, "reset()")
        with pytest.raises(ValueError):
            model.apply(torch.zeros(N, B_ + M + T + 1, device=gpu))
        with pytest.raises(ValueError):
            model.apply(dev, out=torch.zeros(N, B_ + M + T - 1, device=gpu))
        with pytest.raises(ValueError):
            model.apply(dev, torch.zeros(N - 1, dtype=torch.uint8, device=gpu))
        buf = torch.zeros(N, 400, device=gpu)
        with pytest.raises(ValueError, match="overlaps"):
            model.apply(buf[:, :B_ + M + T], out=buf[:, 100:100 + B_ + M + T])
    finally:
        model.close()


def test_captured_apply_equals_host(gpu, S):
    """One apply captured in a graph and replayed three times on fixed buffers equals the host
    statement applied as often: the counters are on the device, so the replays walk the steps and a
    raised flag starts an episode."""
    N, B_, M, T = 65, 1080, 8, 5
    rng = np.random.default_rng(8)
    kw = dict(seed=5, env_offset=100)
    model = S.SensorModel(N, B_, M, T, device=gpu, **kw, **C.active(B_))
    try:
        host = S.host_sensor_state(N)
        rows_dev = torch.zeros(N, B_ + M + T, device=gpu)
        flags = torch.zeros(N, dtype=torch.uint8, device=gpu)
        out = torch.zeros(N, B_ + M + T, device=gpu)
        seq = [(C.rows_for(rng, N, B_, M, T), (rng.random(N) < 0.3).astype(np.uint8) if t == 2 else np.zeros(N, np.uint8))
               for t in range(4)]
        rows_dev.copy_(torch.as_tensor(seq[0][0]))
        model.apply(rows_dev, flags, out=out)  # eager: loads the kernel
        assert C.same_bits(out.cpu().numpy(), S.host_sensor_apply(host, seq[0][0], B_, M, T, reset=seq[0][1], **kw,
                                                                  **C.active(B_)))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.graph(g, stream=side):
            model.apply(rows_dev, flags, out=out)
        torch.cuda.current_stream(gpu).wait_stream(side)
        for t, (rows, reset) in enumerate(seq[1:]):  # three replays
            rows_dev.copy_(torch.as_tensor(rows))
            flags.copy_(torch.as_tensor(reset))
            g.replay()
            want = S.host_sensor_apply(host, rows, B_, M, T, reset=reset, **kw, **C.active(B_))
            assert C.same_bits(out.cpu().numpy(), want), f"replay {t}"
        assert_state(model, host, "after the replays")
        assert host["episode"].max() == 1 and host["step"].max() == 3
    finally:
        model.close()


# ---- F110VectorEnv(sensor_ranges=...) beside a twin without it --------------------------------
ENV_STEPS = 10
RANGES = dict(noise_abs=(0.005, 0.03), noise_rel=(0.0, 0.01), scale=(0.98, 1.02), dropout=(0.0, 0.02), blackout=(0, 30),
              quant=(0.0, 0.01), pose_xy=(0.0, 0.05), pose_theta=(0.0, 0.02))
SOBS = dict(n_bins=36, n_frames=3, stride=2)
MASK = np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8)


def _env(track, **extra):
    from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward
    from f110_gymnasium_ros2_jazzy_amd.train import REWARD_KW
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    rf = BatchedCenterlineReward(8, dt=0.01, progress=track, device=torch.device("cuda:0"), **REWARD_KW)
    return F110VectorEnv(8, num_agents=2, seed=5, device=0, opponent="gap_follow", reward_fn=rf, max_episode_steps=4,
                         infos="minimal", env_offset=16, **extra)


def test_vector_env_beside_its_twin(gpu, S, track):
    """8 envs, two agents, the gap follower, the training reward, a time limit of 4 steps (so every
    env autoresets): rewards, flags, full_obs and the opponent's actions are the twin's bit for bit;
    the returned rows are the host statement over full_obs; with scan_obs behind the stage the host
    push of those corrupted rows; the masked-off envs get full_obs itself."""
    from f110_gymnasium_ros2_jazzy_amd import scan_obs as SO
    sens = dict(sensor_ranges=RANGES, sensor_seed=21, sensor_mask=MASK)
    plain, noisy, both = _env(track), _env(track, **sens), _env(track, scan_obs=SOBS, **sens)
    try:
        W = B + 8
        assert noisy.obs_dim == plain.obs_dim == W and both.obs_dim == 3 * 36 + 8
        with pytest.raises(ValueError):
            plain.sensor_params()
        kw = dict(range_max=30.0, seed=21, env_offset=16, mask=MASK)
        host, ring = S.host_sensor_state(8), SO.host_scan_obs_state(8, B, **SOBS)
        p_obs, _ = plain.reset(seed=9)
        n_obs, _ = noisy.reset(seed=9)
        b_obs, _ = both.reset(seed=9)

        def check(what, reset):
            clean = p_obs.cpu().numpy()
            assert same_bits(noisy.full_obs, p_obs) and same_bits(both.full_obs, p_obs), (what, "full_obs")
            want = S.host_sensor_apply(host, clean, B, 8, reset=reset, **kw, **RANGES)
            assert C.same_bits(n_obs.cpu().numpy(), want), (what, "rows")
            assert C.same_bits(want[6:], clean[6:]) and not C.same_bits(want[:6, :B], clean[:6, :B]), (what, "mask")
            assert (want[:6, B:B + 3] != clean[:6, B:B + 3]).any() and C.same_bits(want[:, B + 3], clean[:, B + 3])
            compact = SO.host_scan_obs_push(ring, want, B, 8, reset=reset, **SOBS)
            assert C.same_bits(b_obs.cpu().numpy(), compact), (what, "compact rows")
        check("reset", None)
        assert C.same_bits(noisy.sensor_params().cpu().numpy(), host["params"])
        rng = np.random.default_rng(1)
        buf = torch.full((8, W), float("nan"), device=gpu)
        cbuf = torch.full((8, both.obs_dim), float("nan"), device=gpu)
        resets = 0
        for k in range(ENV_STEPS):
            a = torch.as_tensor(np.stack([rng.uniform(-0.3, 0.3, 8), rng.uniform(1.0, 6.0, 8)], 1).astype(np.float32),
                                device=gpu)
            p_obs, p_rew, p_term, p_trunc, p_info = plain.step(a)
            if k % 2:  # every other step through step_transition: the rows land in obs_out
                n_obs, n_rew, n_term, n_reset = noisy.step_transition(a, obs_out=buf)
                b_obs, b_rew, b_term, _ = both.step_transition(a, obs_out=cbuf)
                assert n_obs.data_ptr() == buf.data_ptr() and b_obs.data_ptr() == cbuf.data_ptr()
                assert torch.equal(n_term.bool(), p_term) and torch.equal(n_reset.bool(), p_info["reset"])
                assert torch.equal(b_term.bool(), p_term)
                assert same_bits(noisy._act[:, 1], p_info["opponent_actions"]), f"opponent, step {k}"
            else:
                n_obs, n_rew, n_term, n_trunc, n_info = noisy.step(a)
                b_obs, b_rew, b_term, b_trunc, b_info = both.step(a)
                assert torch.equal(n_term, p_term) and torch.equal(n_trunc, p_trunc), f"flags, step {k}"
                assert torch.equal(b_term, p_term) and torch.equal(b_trunc, p_trunc), f"flags, step {k}"
                assert set(n_info) == set(p_info) and torch.equal(n_info["reset"], p_info["reset"])
                for info in (n_info, b_info):
                    assert same_bits(info["opponent_actions"], p_info["opponent_actions"]), f"opponent, step {k}"
            for rew in (n_rew, b_rew):
                assert torch.equal(rew.view(torch.int64), p_rew.view(torch.int64)), f"rewards, step {k}"
            reset = p_info["reset"].cpu().numpy().astype(np.uint8)
            resets += int(reset.sum())
            check(f"step {k}", reset)
        assert resets >= 8  # every env was reset on the device
        assert_state(noisy._sensor, host, "after the run")
        assert host["episode"].min() >= 1
        nxt = noisy.step_transition(a)[0]  # without obs_out: a copy of the env's own sensor rows
        assert nxt.data_ptr() != noisy._noisy.data_ptr() and same_bits(nxt, noisy._noisy)
        n_obs, _ = noisy.reset(seed=3)  # reset() restarts the counters: episode 0 again
        st = noisy._sensor.arrays()
        assert st["episode"].tolist() == [0] * 8 and st["step"].tolist() == [0] * 8
    finally:
        for env in (plain, noisy, both):
            env.close()


def test_train_main_with_sensor_flags(gpu, monkeypatch, capsys):
    """python -m ...train --sensor-noise LO,HI --sensor-dropout LO,HI --eval-envs 2 at 8 envs: the run
    finishes and reports, with the evaluation episodes in the report."""
    import json
    import sys
    from f110_gymnasium_ros2_jazzy_amd import train
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(sys, "argv", ["train", "--envs-per-gpu", "8", "--steps", "500", "--warmup", "3", "--batch", "16",
                                      "--memory", "1024", "--max-episode-steps", "40", "--sensor-noise", "0.005,0.03",
                                      "--sensor-dropout", "0,0.02", "--eval-envs", "2"])
    train.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["step"] == 500 and line["obs_dim"] == B + 8
    assert line["critic_loss"] is not None and np.isfinite(line["critic_loss"])
    assert line["episodes"] > 0 and line["eval_episodes"] > 0


def test_trainer_masks_the_eval_rows(gpu, monkeypatch):
    """VectorTrainer(sensor_ranges=..., eval_envs=2): the last two rows of the observation are the
    clean rows, the others are not; step graphs on."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    monkeypatch.setenv("F110_STEP_GRAPH", "1")
    tr = VectorTrainer(16, batch_size=16, memory_size=256, warmup_steps=2, seed=3, eval_envs=2, max_episode_steps=5,
                       sensor_ranges=dict(noise_abs=(0.005, 0.03), dropout=(0.0, 0.02)))
    try:
        for k in range(10):
            tr.step()
            full = tr.env.full_obs
            assert same_bits(tr.obs[14:], full[14:]), f"eval rows, step {k}"
            assert not same_bits(tr.obs[:14, :B], full[:14, :B]), f"training rows, step {k}"
            assert same_bits(tr.obs[:, B:], full[:, B:])  # no pose noise asked for
        torch.cuda.synchronize()
        assert tr.env._sensor.mask.tolist() == [1] * 14 + [0, 0]
        assert tr.last is not None and np.isfinite(float(tr.last["critic_loss"]))
    finally:
        tr.close()
