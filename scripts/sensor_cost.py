"""What the sensor randomization costs (GPU box), one JSON line per measurement.

    python scripts/sensor_cost.py kernel [every | flags | identity]   # for a kernel trace of one set of ranges:
                                                # rocprofv3 --kernel-trace --stats -- python ... kernel every
    python scripts/sensor_cost.py trainer
    python scripts/sensor_cost.py off           # F110_TREE=<a checkout of another commit>: that tree's package

kernel   SensorModel(4096, 1080, 8, 0) over rows [4096, 1088]: 20 applies of warm-up, then 500
         back-to-back applies between two device events, for every parameter active, for the trainer's
         two flags (noise_abs, dropout) and for the identity (no draw is computed), each into a
         disjoint buffer and in place; and 500 plain device copies of the same rows into the same
         buffer (torch's copy_) in the same process.  Under the profiler k_sensor's own time is in the
         trace beside the copy kernel's.
trainer  env-steps/s of the graphed trainer (the shape of bench.py --workload ddpg) with the stage
         off (two trainers: their difference is the spread) and on (the two flags of
         `train.py --sensor-noise 0.005,0.03 --sensor-dropout 0,0.02`, and every parameter),
         interleaved rounds whose order rotates.
off      the two stage-off trainers alone: what another tree (F110_TREE) is compared by.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("F110_TREE") or REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

E = int(os.environ.get("SENSOR_ENVS", 4096))
FLAGS = dict(noise_abs=(0.005, 0.03), dropout=(0.0, 0.02))
EVERY = dict(noise_abs=(0.005, 0.03), noise_rel=(0.0, 0.01), scale=(0.98, 1.02), dropout=(0.0, 0.02), blackout=(0, 30),
             quant=(0.0, 0.01), pose_xy=(0.0, 0.05), pose_theta=(0.0, 0.02))


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us


def kernel_run(only=None):
    from f110_gymnasium_ros2_jazzy_amd.sensor import SensorModel
    dev = torch.device("cuda:0")
    B, M = 1080, 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    rows = torch.rand(E, B + M, generator=gen, device=dev)
    out = torch.empty_like(rows)
    res = {"mode": "kernel", "envs": E, "width": B + M, "bytes_moved": 2 * rows.numel() * 4, "apply_us": {}}
    for name, ranges in (("every", EVERY), ("flags", FLAGS), ("identity", {})):
        if only not in (None, name):
            continue
        model = SensorModel(E, B, M, 0, seed=5, device=dev, **ranges)
        for dst, tag in ((out, "disjoint"), (rows, "in_place")):
            for _ in range(20):
                model.apply(rows, out=dst)
            torch.cuda.synchronize()
            res["apply_us"][f"{name}_{tag}"] = [events(lambda: model.apply(rows, out=dst), 500) for _ in range(3)]
            rows.uniform_(0.0, 1.0, generator=gen)
        model.close()
    for _ in range(20):
        out.copy_(rows)
    torch.cuda.synchronize()
    res["copy_us"] = [events(lambda: out.copy_(rows), 500) for _ in range(3)]
    print(json.dumps(res), flush=True)


def trainer_run(shapes):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    rounds, K = int(os.environ.get("SENSOR_ROUNDS", 6)), int(os.environ.get("SENSOR_STEPS", 200))
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
    print(json.dumps({"mode": "trainer", "tree": os.environ.get("F110_TREE") or REPO, "envs": E, "rounds": rounds,
                      "steps_per_round": K, "step_ms": step, "step_ms_rounds": times,
                      "env_steps_per_s": {m: E / (v * 1e-3) for m, v in step.items()},
                      "step_graphs": {m: sorted(map(str, tr._sg)) for m, tr in trs.items()}}), flush=True)
    for tr in trs.values():
        tr.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "trainer"
    if mode == "kernel":
        kernel_run(sys.argv[2] if len(sys.argv) > 2 else None)
    elif mode == "off":
        trainer_run({"off_a": {}, "off_b": {}})
    else:
        trainer_run({"off_a": {}, "off_b": {}, "flags": dict(sensor_ranges=FLAGS), "every": dict(sensor_ranges=EVERY)})
