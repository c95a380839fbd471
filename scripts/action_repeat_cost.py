"""What action repeat changes in a trainer step (GPU box): the per-step time of VectorTrainer at
4096 two-agent envs (batch 4096, step graphs) with action_repeat 1 and 4, both trainers alive in
one process and timed in interleaved rounds whose order alternates.  K = 4 adds one hold launch
before the env step and replaces the 4096-row ring add by the four push launches, which move about
a quarter of the rows; the actor, the simulator and the learner update run at every step either way.

Per trainer the median over rounds of a round's mean step time (host clock around K steps that end
in a synchronise), and the spread (min .. max) over the rounds.  Prints one JSON line.

    python scripts/action_repeat_cost.py
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
    E = int(os.environ.get("REPEAT_ENVS", 4096))
    batch = int(os.environ.get("REPEAT_BATCH", 4096))
    rounds = int(os.environ.get("REPEAT_ROUNDS", 6))
    K = int(os.environ.get("REPEAT_STEPS", 200))
    repeats = [1, int(os.environ.get("REPEAT_K", 4))]
    limit = int(os.environ.get("REPEAT_MAX_EPISODE_STEPS", 1000))
    trs = {r: VectorTrainer(E, batch_size=batch, memory_size=1 << 18, warmup_steps=2, seed=7, action_repeat=r,
                            max_episode_steps=limit) for r in repeats}
    for tr in trs.values():  # the warm-up, the learner's eager updates, both parities' captures, first replays
        for _ in range(40):
            tr.step()
    torch.cuda.synchronize()
    times = {r: [] for r in repeats}
    for rd in range(rounds):
        for r in (repeats if rd % 2 == 0 else repeats[::-1]):
            tr = trs[r]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                tr.step()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) / K * 1e3)
    step = {r: float(np.median(v)) for r, v in times.items()}
    rows = {r: len(tr.agent.memory) for r, tr in trs.items()}
    a, b = repeats
    res = {"envs": E, "batch": batch, "rounds": rounds, "steps_per_round": K, "max_episode_steps": limit,
           "step_ms": {str(r): v for r, v in step.items()},
           "step_ms_spread": {str(r): [min(v), max(v)] for r, v in times.items()},
           "step_ms_rounds": {str(r): v for r, v in times.items()},
           "added_ms": step[b] - step[a], "ratio": step[b] / step[a],
           "stored_rows": {str(r): v for r, v in rows.items()},
           "critic_loss": {str(r): float(tr.last["critic_loss"]) for r, tr in trs.items()},
           "step_graphs": {str(r): sorted(map(str, tr._sg)) for r, tr in trs.items()}}
    for tr in trs.values():
        tr.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
