"""What the per-env parameter table costs a step (GPU box): 65536 single-agent envs on one context
(Spielberg, noise and autoreset on, random resident actions), stepped with no table, with a table
(f110_set_env_params) and with domain randomization on top (f110_set_param_randomization).

    python scripts/env_params_cost.py                 # the three in alternating rounds: step rates, one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python scripts/env_params_cost.py table
                                                      # one mode only (none | table | rand), for the kernel stats:
                                                      # k_agents<false, false> against k_agents<false, true>
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd.maps import centerline_spawns, load_map  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.sim import BatchSim  # noqa: E402

RANGES = {"mu": (0.6, 1.1), "m": (3.0, 4.5), "C_Sf": (3.8, 5.6), "C_Sr": (4.4, 6.5), "a_max": (7.0, 11.0)}


def main():
    modes = sys.argv[1:] or ["none", "table", "rand"]
    E = int(os.environ.get("EP_ENVS", 65536))
    steps = int(os.environ.get("EP_STEPS", 300))
    rounds = int(os.environ.get("EP_ROUNDS", 3))
    dev = torch.device("cuda:0")
    tm = load_map("Spielberg_map")
    tm.ensure_edt()
    sp = centerline_spawns("Spielberg", 1)
    rng = np.random.default_rng(12345)
    poses = sp[rng.integers(0, sp.shape[0], E)]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    acts = torch.rand(steps, E, 1, 2, device=dev, generator=g)
    acts[..., 0] = acts[..., 0] * 0.8378 - 0.4189
    acts[..., 1] *= 20
    sims = {}
    for m in modes:
        sm = BatchSim(tm, n_envs=E, n_agents=1, device=dev, noise_std=0.01, autoreset=True, spawn_poses=sp, seed=7)
        if m == "table":
            sm.set_env_params({k: rng.uniform(lo, hi, E) for k, (lo, hi) in RANGES.items()})
        elif m == "rand":
            sm.set_param_randomization(RANGES, seed=3)
        sm.reset(poses)
        sims[m] = sm
    ms = {m: [] for m in modes}
    resets = {}
    for _ in range(rounds):
        for m, sm in sims.items():
            sm.reset(poses)
            for k in range(30):
                sm.step(acts[k], minimal_outputs=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                sm.step(acts[k], minimal_outputs=True)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / steps * 1e3)
            if m not in resets:  # how many cars a step resets (each redraws its row under "rand"); not timed
                nres = torch.zeros((), dtype=torch.int64, device=dev)
                for k in range(100):
                    nres += sm.step(acts[k]).was_reset.sum()
                resets[m] = int(nres) / 100
    out = {"envs": E, "steps": steps, "rounds": rounds}
    for m in modes:
        out[m] = {"step_ms": ms[m], "median_step_ms": float(np.median(ms[m])),
                  "env_steps_per_s": E / (float(np.median(ms[m])) * 1e-3), "autoresets_per_step": resets[m]}
    print(json.dumps(out), flush=True)
    for sm in sims.values():
        sm.close()


if __name__ == "__main__":
    main()
