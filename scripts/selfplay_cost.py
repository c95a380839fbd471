"""What self-play adds to a trainer step (GPU box): the per-step time of VectorTrainer at 4096
two-agent envs (batch 4096, step graphs) with the gap-follow opponent and with --opponent self,
both trainers alive in one process and timed in interleaved rounds whose order alternates; and the
achieved bytes/s of f110_agent_obs alone at the same shape, against a float4 device-to-device copy
of the same bytes and the measured HBM copy rate of MI355X_MICROARCH (6.29 TB/s).

Per trainer the median over rounds of a round's mean step time (host clock around K steps that end
in a synchronise).  The pack's bytes: E x (B + 4A) floats read and as many written; its time:
device events around R back-to-back launches.  Prints one JSON line.

    python scripts/selfplay_cost.py
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd.opponent import agent_obs  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the device's HBM


def events_ms(fn, reps):
    """Mean time of one fn() over reps back-to-back calls (device events, read once at the end)."""
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pack_rate(E, A=2, B=1080, reps=200, rounds=5):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    W = B + 4 * A
    # a ring of buffer sets larger than the 256 MiB Infinity Cache, so every launch reads from HBM
    sets = max(2, int((512 << 20) // (E * (A * B + 2 * W) * 4)) + 1)
    scans = [torch.rand(E, A, B, device=dev, generator=g) * 31.0 for _ in range(sets)]
    obs = [torch.rand(E, W, device=dev, generator=g) for _ in range(sets)]
    out = [torch.empty(E, W, device=dev) for _ in range(sets)]
    k = [0]

    def pack():
        i = k[0] % sets
        agent_obs(scans[i], obs[i], 1, 30.0, out=out[i])
        k[0] += 1

    def copy():  # the same bytes each way through torch's contiguous float copy
        i = k[0] % sets
        out[i].copy_(obs[i])
        k[0] += 1

    for fn in (pack, copy):
        events_ms(fn, 20)
    ms = {"agent_obs": [], "copy": []}
    for _ in range(rounds):
        ms["agent_obs"].append(events_ms(pack, reps))
        ms["copy"].append(events_ms(copy, reps))
    nbytes = 2 * E * W * 4
    res = {"envs": E, "bytes_per_launch": nbytes, "buffer_sets": sets}
    for n, v in ms.items():
        m = float(np.median(v))
        res[n] = {"ms": m, "ms_rounds": v, "TB_per_s": nbytes / (m * 1e-3) / 1e12,
                  "share_of_hbm_copy_rate": nbytes / (m * 1e-3) / 1e12 / HBM_COPY_TBS}
    return res


def main():
    E = int(os.environ.get("SELFPLAY_ENVS", 4096))
    batch = int(os.environ.get("SELFPLAY_BATCH", 4096))
    rounds = int(os.environ.get("SELFPLAY_ROUNDS", 6))
    K = int(os.environ.get("SELFPLAY_STEPS", 200))
    sync = int(os.environ.get("SELFPLAY_SYNC", 1000))
    kinds = ["gap_follow", "self"]
    trs = {n: VectorTrainer(E, batch_size=batch, memory_size=1 << 18, warmup_steps=2, seed=7, opponent=n,
                            selfplay_sync=sync) for n in kinds}
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
    res = {"envs": E, "batch": batch, "rounds": rounds, "steps_per_round": K, "selfplay_sync": sync,
           "step_ms": step, "step_ms_rounds": times, "added_ms": step["self"] - step["gap_follow"],
           "ratio": step["self"] / step["gap_follow"],
           "step_graphs": {n: sorted(map(str, tr._sg)) for n, tr in trs.items()}}
    for tr in trs.values():
        tr.close()
    res["agent_obs"] = pack_rate(E)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
