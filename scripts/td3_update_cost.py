"""The learner update's time for DDPG and TD3 (GPU box), events around replay() as bench.py's
phases_ms.learner_update_ms takes them: batch 4096, obs 1088, one device, the learner's own HIP
graphs (graphs=True), a full replay ring of random rows.

  ddpg        the default learner on this build
  ddpg_alt    the same Python on an alternate libf110 build (AB_LIB, e.g. the parent commit's
              library), loaded into the same process and timed in interleaved rounds whose
              order rotates
  td3         algo="td3", policy_delay 2: critic-only updates and actor-step updates timed
              separately, and their mean

Per learner the median over rounds of the mean update time of a round.  Prints one JSON line.

    AB_LIB=ab_libs/parent.so python scripts/td3_update_cost.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd import _build, _lib  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner  # noqa: E402

LOW, HIGH = [-0.4189, 0.0], [0.4189, 20.0]


def load_lib(path):
    _lib._lib = None
    if path == _build.LIB:
        os.environ.pop("F110_LIB", None)
    else:
        os.environ["F110_LIB"] = path
    L = _lib.load(build_if_missing=False)
    _lib._lib = None
    os.environ.pop("F110_LIB", None)
    return L


def with_lib(L, fn):
    _lib._lib = L
    try:
        return fn()
    finally:
        _lib._lib = None


def main():
    M = int(os.environ.get("TD3_BATCH", 4096))
    D = int(os.environ.get("TD3_OBS", 1088))
    rounds = int(os.environ.get("TD3_ROUNDS", 6))  # (a multiple of the learners: every order equally often)
    K = int(os.environ.get("TD3_UPDATES", 100))  # per round (even: both TD3 kinds equally often)
    dev = torch.device("cuda:0")
    libs = {"ddpg": _build.LIB, "td3": _build.LIB}
    if os.environ.get("AB_LIB"):
        libs["ddpg_alt"] = os.path.join(REPO, os.environ["AB_LIB"])
    if os.environ.get("TD3_REVERSE") == "1":  # build the learners (their allocations) in the other order
        libs = dict(reversed(list(libs.items())))
    Ls = {n: load_lib(p) for n, p in libs.items()}
    g = torch.Generator(device=dev).manual_seed(0)
    cap = 1 << 15
    S = torch.rand(cap, D, device=dev, generator=g)
    A = torch.rand(cap, 2, device=dev, generator=g) * torch.tensor([0.8378, 20.0], device=dev) - \
        torch.tensor([0.4189, 0.0], device=dev)
    R = torch.randn(cap, device=dev, generator=g)
    S2 = torch.rand(cap, D, device=dev, generator=g)
    Dn = torch.rand(cap, device=dev, generator=g) < 0.05
    lns = {}
    for n, L in Ls.items():
        def make(n=n):
            ln = DDPGLearner(obs_dim=D, act_dim=2, action_low=LOW, action_high=HIGH, seed=3, device=dev,
                             memory_size=cap, batch_size=M, graphs=True, max_add=cap,
                             algo="td3" if n == "td3" else "ddpg", policy_delay=2)
            ln.remember(S, A, R, S2, Dn)
            for _ in range(10):  # eager warm-up, captures of both update kinds, first replays
                ln.replay()
            return ln
        lns[n] = with_lib(L, make)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    times = {n: [] for n in lns}
    kinds = {"critic_only": [], "actor_step": []}
    names = list(lns)
    for rd in range(rounds):
        for n in names[rd % len(names):] + names[:rd % len(names)]:  # the order rotates: no learner always runs first
            ln = lns[n]
            evs, actor = [], []
            for _k in range(K):  # submitted back to back, the events read once at the end
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                actor.append(ln.is_actor_step())
                e0.record(stream)
                with_lib(Ls[n], ln.replay)
                e1.record(stream)
                evs.append((e0, e1))
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in evs])
            times[n].append(float(ms.mean()))
            if n == "td3":
                act = np.array(actor)
                kinds["critic_only"].append(float(ms[~act].mean()))
                kinds["actor_step"].append(float(ms[act].mean()))
    res = {"batch": M, "obs_dim": D, "rounds": rounds, "updates_per_round": K, "libs": libs,
           "update_ms": {n: float(np.median(v)) for n, v in times.items()},
           "update_ms_rounds": times,
           "td3_ms": {k: float(np.median(v)) for k, v in kinds.items()}}
    base = res["update_ms"]["ddpg"]
    res["ratio_to_ddpg"] = {"td3_mean": res["update_ms"]["td3"] / base,
                            **{k: v / base for k, v in res["td3_ms"].items()},
                            **({"ddpg_alt": res["update_ms"]["ddpg_alt"] / base} if "ddpg_alt" in lns else {})}
    for ln in lns.values():
        ln.memory.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
