"""What the episode limits cost a step (GPU box): BatchSim.step on one context (Spielberg, noise and
autoreset on, random resident actions, full outputs: the stats read was_reset) three ways, in alternating rounds:

    off       no limits (the limit-free epilogue)
    on        f110_set_episode_limits(max_steps, stall_speed, stall_steps): the epilogue's extra [E]
              stall-counter load + store, the ego speed load and the u8 flag store
    on_stats  the same plus f110_episode_stats on the step's flags and a constant reward (two
              small launches)

    python scripts/episode_limits_cost.py                       # 65536x1 and 8192x2, one JSON line
    python scripts/episode_limits_cost.py --shapes 4096x1 --steps 200 --rounds 5
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd.episode import EpisodeStats  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.maps import centerline_spawns, load_map  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim  # noqa: E402

MODES = ("off", "on", "on_stats")


def run_shape(E, A, args, dev, tm):
    sp = centerline_spawns("Spielberg", A)
    rng = np.random.default_rng(12345)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    acts = torch.rand(args.steps, E, A, 2, device=dev, generator=g)
    acts[..., 0] = acts[..., 0] * 0.8378 - 0.4189
    acts[..., 1] *= 20
    rewards = torch.full((E,), 0.01, dtype=torch.float64, device=dev)
    sims, stats = {}, None
    for m in MODES:
        sm = BatchSim(tm, n_envs=E, n_agents=A, device=dev, noise_std=0.01, autoreset=True, spawn_poses=sp, seed=7)
        if m != "off":
            sm.set_episode_limits(args.max_steps, args.stall_speed, args.stall_steps)
        sims[m] = sm
    stats = EpisodeStats(E, device=dev)
    ms = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m, sm in sims.items():
            sm.reset(poses)
            stats.reset()

            def step(k):
                o = sm.step(acts[k])
                if m == "on_stats":
                    stats.update(rewards, o.terminated, o.truncated, o.was_reset)
            for k in range(min(30, args.steps)):
                step(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                step(k)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"envs": E, "agents": A}
    for m in MODES:
        med = float(np.median(ms[m]))
        out[m] = {"step_ms": [round(x, 5) for x in ms[m]], "median_step_ms": med, "env_steps_per_s": E / (med * 1e-3)}
    out["on_minus_off_ms"] = out["on"]["median_step_ms"] - out["off"]["median_step_ms"]
    out["stats_minus_on_ms"] = out["on_stats"]["median_step_ms"] - out["on"]["median_step_ms"]
    t = stats.totals()
    out["episodes_in_stats"] = t["episodes"]
    for sm in sims.values():
        sm.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="65536x1,8192x2", help="comma-separated ENVSxAGENTS")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--stall-speed", type=float, default=0.1)
    ap.add_argument("--stall-steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tm = load_map("Spielberg_map")
    tm.ensure_edt()
    res = []
    for s in args.shapes.split(","):
        E, A = (int(x) for x in s.lower().split("x"))
        res.append(run_shape(E, A, args, dev, tm))
    print(json.dumps({"steps": args.steps, "rounds": args.rounds, "max_steps": args.max_steps,
                      "stall_speed": args.stall_speed, "stall_steps": args.stall_steps, "shapes": res}), flush=True)


if __name__ == "__main__":
    main()
