"""What the pure-pursuit opponent costs (GPU box).

Per call, at 4096 and 8192 rows, in one process and from the on-track poses of a stepped env
(two agents, both driven by the pursuit for PURSUIT_SETTLE steps after a spawn-table reset):
f110_pure_pursuit (k_pursuit) on the opponent's pose group of the obs, beside f110_gap_follow on the
opponent's scans and f110_reward (k_reward, the yardstick: it projects two points per env where the
pursuit projects one) on the same obs.  Device events around one replay of a HIP graph of R
back-to-back launches (no host work between them), the three kernels in interleaved rounds; the
median over rounds.

Per trainer step: VectorTrainer at 4096 two-agent envs (batch 4096, step graphs) with the gap-follow
opponent and with opponent="pure_pursuit", both alive in one process and timed in interleaved
rounds whose order alternates (the median over rounds of a round's mean step time, host clock around
K steps that end in a synchronise).  Prints one JSON line.

    python scripts/pursuit_cost.py
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd.maps import MAP_DIR  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.opponent import gap_follow, pure_pursuit  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward, CenterlineTrack  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.train import REWARD_KW, VectorTrainer  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv  # noqa: E402


def capture(fn, reps):
    """reps back-to-back fn() launches as one HIP graph: a replay has no host work between the
    launches, so a call of a few microseconds is not timed at the Python wrapper's pace."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_ms(g, reps):
    """Mean time of one launch of a captured chain of reps (device events around one replay)."""
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    g.replay()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_cost(track, rows, settle, reps=200, rounds=7):
    dev = torch.device("cuda:0")
    env = F110VectorEnv(rows, num_agents=2, seed=7, device=dev, opponent="pure_pursuit", opponent_track=track,
                        infos="minimal")
    B = env.sim.B
    obs, _ = env.reset(seed=7)
    crashed = torch.zeros(rows, dtype=torch.bool, device=dev)
    for _ in range(settle):
        obs, _, term, _, _ = env.step(pure_pursuit(obs[:, B:B + 4], track))
        crashed |= term
    scans = env.sim.out.scans.clone()
    obs = obs.clone()
    reward = BatchedCenterlineReward(rows, dt=0.01, progress=track, device=dev, **REWARD_KW)
    act = torch.zeros(rows, 2, 2, device=dev)
    fns = {"pure_pursuit": lambda: pure_pursuit(obs[:, B + 4:B + 8], track, out=act[:, 1]),
           "gap_follow": lambda: gap_follow(scans[:, 1], out=act[:, 1]),
           "reward": lambda: reward(obs)}
    for fn in fns.values():  # first launches load the code objects
        fn()
    torch.cuda.synchronize()
    graphs = {n: capture(fn, reps) for n, fn in fns.items()}
    ms = {n: [] for n in fns}
    for _ in range(rounds):
        for n, g in graphs.items():
            ms[n].append(replay_ms(g, reps))
    _, aux = pure_pursuit(obs[:, B + 4:B + 8], track, return_aux=True)
    res = {"rows": rows, "settle_steps": settle, "crashed_while_settling": int(crashed.sum()),
           "max_abs_t": float(aux[:, 1].abs().max()),
           "us": {n: float(np.median(v)) * 1e3 for n, v in ms.items()},
           "us_rounds": {n: [x * 1e3 for x in v] for n, v in ms.items()}}
    res["pursuit_over_reward"] = res["us"]["pure_pursuit"] / res["us"]["reward"]
    env.close()
    return res


def trainer_cost(E, batch, rounds, K):
    kinds = ["gap_follow", "pure_pursuit"]
    trs = {n: VectorTrainer(E, batch_size=batch, memory_size=1 << 18, warmup_steps=2, seed=7, opponent=n)
           for n in kinds}
    for tr in trs.values():  # the warm-up, the learner's eager updates, both parities' captures, first replays
        for _ in range(40):
            tr.step()
    torch.cuda.synchronize()
    times = {n: [] for n in kinds}
    for rd in range(rounds):
        for n in (kinds if rd % 2 == 0 else kinds[::-1]):
            tr = trs[n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                tr.step()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / K * 1e3)
    step = {n: float(np.median(v)) for n, v in times.items()}
    res = {"envs": E, "batch": batch, "rounds": rounds, "steps_per_round": K, "step_ms": step,
           "step_ms_rounds": times, "added_ms": step["pure_pursuit"] - step["gap_follow"],
           "ratio": step["pure_pursuit"] / step["gap_follow"],
           "step_graphs": {n: sorted(map(str, tr._sg)) for n, tr in trs.items()}}
    for tr in trs.values():
        tr.close()
    return res


def main():
    settle = int(os.environ.get("PURSUIT_SETTLE", 300))
    cl = np.load(os.path.join(MAP_DIR, "Spielberg_centerline.npz"))
    track = CenterlineTrack(cl["xy"], cl["w_right"], cl["w_left"], device=0)
    res = {"kernels": [kernel_cost(track, rows, settle) for rows in (4096, 8192)]}
    track.close()
    if os.environ.get("PURSUIT_TRAINER", "1") != "0":
        res["trainer"] = trainer_cost(int(os.environ.get("PURSUIT_ENVS", 4096)),
                                      int(os.environ.get("PURSUIT_BATCH", 4096)),
                                      int(os.environ.get("PURSUIT_ROUNDS", 6)), int(os.environ.get("PURSUIT_STEPS", 200)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
