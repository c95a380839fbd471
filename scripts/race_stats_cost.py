"""What the race statistics cost a trainer step (GPU box): the per-step time of VectorTrainer at
4096 two-agent envs (batch 4096, step graphs, the shape of bench.py --workload ddpg) with race_stats
off and on.  Three trainers live in one process -- two with the flag off, whose difference is the
run-to-run spread a figure has to beat, and one with it on -- and are timed in interleaved rounds
whose order rotates.  With the flag on every step graph holds three more launches after the reward
(k_race_project: one wave per env, k_race, k_race_finish); with it off the launch sequence is the
one without the feature.

Per trainer the median over rounds of a round's mean step time (host clock around K steps that end
in a synchronise), and the spread (min .. max) over the rounds.  Prints one JSON line.

    python scripts/race_stats_cost.py
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer  # noqa: E402


def main():
    E = int(os.environ.get("RACE_ENVS", 4096))
    batch = int(os.environ.get("RACE_BATCH", 4096))
    rounds = int(os.environ.get("RACE_ROUNDS", 6))
    K = int(os.environ.get("RACE_STEPS", 200))
    modes = {"off_a": False, "off_b": False, "on": True}
    trs = {m: VectorTrainer(E, batch_size=batch, memory_size=1 << 18, warmup_steps=2, seed=7, race_stats=on)
           for m, on in modes.items()}
    for tr in trs.values():  # the warm-up, the learner's eager updates, both parities' captures, first replays
        for _ in range(40):
            tr.step()
    torch.cuda.synchronize()
    names = list(modes)
    times = {m: [] for m in names}
    for rd in range(rounds):
        for m in names[rd % 3:] + names[:rd % 3]:
            tr = trs[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                tr.step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / K * 1e3)
    step = {m: float(np.median(v)) for m, v in times.items()}
    off = 0.5 * (step["off_a"] + step["off_b"])
    race = trs["on"].env.race_totals()
    res = {"envs": E, "batch": batch, "rounds": rounds, "steps_per_round": K,
           "step_ms": step, "step_ms_spread": {m: [min(v), max(v)] for m, v in times.items()},
           "step_ms_rounds": times,
           "off_spread_ms": abs(step["off_a"] - step["off_b"]),
           "added_ms": step["on"] - off, "ratio": step["on"] / off,
           "env_steps_per_s": {m: E / (v * 1e-3) for m, v in step.items()},
           "race_totals": {k: race[k] for k in ("episodes", "progress_mean", "lead_mean", "win_rate", "crash_rate",
                                                "passes", "passed")},
           "step_graphs": {m: sorted(map(str, tr._sg)) for m, tr in trs.items()}}
    for tr in trs.values():
        tr.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
