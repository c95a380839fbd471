"""What the scan observation costs and saves (GPU box), three measurements, one JSON line each.

    python scripts/scan_obs_cost.py env 108 1 1     # for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...
    python scripts/scan_obs_cost.py learner
    python scripts/scan_obs_cost.py trainer

env K F S   F110VectorEnv(4096, num_agents=2, opponent="gap_follow", reward_fn=..., track_obs=True,
            scan_obs={n_bins: K, n_frames: F, stride: S}, max_episode_steps=200): a reset and 200
            step_transition calls with random ego actions, then 500 back-to-back ScanObs.push launches
            between two device events.  Run under the profiler, k_scan_obs, k_track_obs and k_reward
            are in one trace.
learner     the learner update at obs_dim 1088 against the compact widths (--scan-bins 108, and
            --scan-bins 36 --scan-frames 3 --scan-stride 2): VectorTrainer(4096, batch_size=4096,
            memory_size=65536), step graphs off, 12 trainer steps, 20 agent.replay() calls of warm-up,
            then 200 between two device events, and 100 eager trainer steps between events; the
            trainers alternately, twice.
trainer     env-steps/s of the graphed trainer (the shape of bench.py --workload ddpg) with the
            feature off (two trainers: their difference is the spread) and on (the two shapes),
            interleaved rounds whose order rotates.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

E = int(os.environ.get("SCAN_ENVS", 4096))
SHAPES = {"k108": dict(scan_bins=108), "k36f3s2": dict(scan_bins=36, scan_frames=3, scan_stride=2)}


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us


def env_run(K, F, S):
    from f110_gymnasium_ros2_jazzy_amd.maps import MAP_DIR
    from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward, CenterlineTrack
    from f110_gymnasium_ros2_jazzy_amd.train import REWARD_KW
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    dev = torch.device("cuda:0")
    cl = np.load(os.path.join(MAP_DIR, "Spielberg_centerline.npz"))
    track = CenterlineTrack(cl["xy"], cl["w_right"], cl["w_left"], device=0)
    rf = BatchedCenterlineReward(E, dt=0.01, progress=track, device=dev, **REWARD_KW)
    env = F110VectorEnv(E, num_agents=2, opponent="gap_follow", reward_fn=rf, infos="minimal", device=dev, seed=7,
                        track_obs=True, scan_obs=dict(n_bins=K, n_frames=F, stride=S), max_episode_steps=200)
    env.reset(seed=1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    buf = torch.empty(E, env.obs_dim, device=dev)
    for _ in range(200):
        u = torch.rand(E, 2, generator=gen, device=dev)
        env.step_transition(torch.stack([(u[:, 0] - 0.5) * 0.6, 1.0 + 5.0 * u[:, 1]], 1), obs_out=buf)
    torch.cuda.synchronize()
    full, flags = env.full_obs, env.sim.out.was_reset
    us = events(lambda: env._sobs.push(full, reset=flags, out=buf), 500)
    print(json.dumps({"mode": "env", "envs": E, "n_bins": K, "n_frames": F, "stride": S, "obs_dim": env.obs_dim,
                      "full_width": int(full.shape[1]), "push_us_back_to_back": us}), flush=True)
    env.close()
    track.close()


def learner_run():
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    os.environ["F110_STEP_GRAPH"] = "0"
    shapes = {"full": {}, **SHAPES}
    trs = {m: VectorTrainer(E, batch_size=4096, memory_size=65536, warmup_steps=4, seed=7, **kw)
           for m, kw in shapes.items()}
    for tr in trs.values():
        for _ in range(12):
            tr.step()
        for _ in range(20):
            tr.agent.replay()
    torch.cuda.synchronize()
    res = {"mode": "learner", "envs": E, "obs_dim": {m: tr.agent.obs_dim for m, tr in trs.items()},
           "update_us": {m: [] for m in trs}, "eager_step_us": {m: [] for m in trs}}
    for _ in range(2):
        for m, tr in trs.items():
            res["update_us"][m].append(events(tr.agent.replay, 200))
        for m, tr in trs.items():
            res["eager_step_us"][m].append(events(tr.step, 100))
    for tr in trs.values():
        tr.close()
    print(json.dumps(res), flush=True)


def trainer_run():
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    rounds, K = int(os.environ.get("SCAN_ROUNDS", 6)), int(os.environ.get("SCAN_STEPS", 200))
    shapes = {"off_a": {}, "off_b": {}, **SHAPES}
    trs = {m: VectorTrainer(E, batch_size=4096, memory_size=1 << 18, warmup_steps=2, seed=7, **kw)
           for m, kw in shapes.items()}
    for tr in trs.values():  # the warm-up, the learner's eager updates, both parities' captures, first replays
        for _ in range(40):
            tr.step()
    torch.cuda.synchronize()
    names = list(shapes)
    times = {m: [] for m in names}
    for rd in range(rounds):
        k = rd % len(names)
        for m in names[k:] + names[:k]:
            tr = trs[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                tr.step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / K * 1e3)
    step = {m: float(np.median(v)) for m, v in times.items()}
    print(json.dumps({"mode": "trainer", "envs": E, "rounds": rounds, "steps_per_round": K,
                      "obs_dim": {m: tr.agent.obs_dim for m, tr in trs.items()}, "step_ms": step,
                      "step_ms_rounds": times, "env_steps_per_s": {m: E / (v * 1e-3) for m, v in step.items()},
                      "step_graphs": {m: sorted(map(str, tr._sg)) for m, tr in trs.items()}}), flush=True)
    for tr in trs.values():
        tr.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "trainer"
    if mode == "env":
        env_run(*(int(x) for x in sys.argv[2:5]))
    elif mode == "learner":
        learner_run()
    else:
        trainer_run()
