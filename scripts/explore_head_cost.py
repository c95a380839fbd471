"""What the per-row exploration head costs a launch (GPU box): the actor's last layer at B x K -> nout,
three ways in one process, in alternating rounds:

    explore       f110_ddpg_actor_explore (the Gaussian head the default trainer launches)
    env_gauss     f110_ddpg_actor_explore_env, kind 0, no masks (the same draws and actions)
    env_ou_masks  f110_ddpg_actor_explore_env, kind 1 (OU: one f64 state read-modify-write per row
                  and output) with an eval mask (the last B / 8 rows) and a reset mask (every 16th row)

Each round times `launches` back-to-back launches per mode twice: issued eagerly (device events
around them: launch overhead included) and as one captured graph of them (the kernels with the
graph's node gaps only).  Prints one JSON line: microseconds per launch, median over the rounds.

    python scripts/explore_head_cost.py                    # 4096 x 128 -> 2
    python scripts/explore_head_cost.py --rows 65536 --launches 100
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from f110_gymnasium_ros2_jazzy_amd import _lib  # noqa: E402
from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import _p, _stream, actor_explore_env  # noqa: E402

MODES = ("explore", "env_gauss", "env_ou_masks")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nout", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.load()
    B, K, n = args.rows, args.hidden, args.nout
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(B, K, device=dev, generator=g).relu()
    W = torch.randn(n, K, device=dev, generator=g) * 0.1
    b = torch.zeros(n, device=dev)
    low = torch.tensor([-0.4189, 0.0, -1.0, -1.0][:n], device=dev)
    high = torch.tensor([0.4189, 20.0, 1.0, 1.0][:n], device=dev)
    scale, shift = 0.5 * (high - low), 0.5 * (high + low)
    pair = torch.tensor([[0.2, 0.0], [0.2, 0.0]], dtype=torch.float64, device=dev)
    out = torch.empty(B, 2, n, device=dev)[:, 0]  # a strided view, as the env's action rows
    ou_x = torch.zeros(B, n, dtype=torch.float64, device=dev)
    i = torch.arange(B, device=dev)
    ev = (i >= B - B // 8).to(torch.uint8)
    rs = (i % 16 == 0).to(torch.uint8)

    def launch(mode, k):
        s_in, s_out = pair[k & 1], pair[1 - (k & 1)]
        if mode == "explore":
            _lib.check(L.f110_ddpg_actor_explore(_p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, n, _p(s_in),
                                                 _p(s_out), 0.9995, 0.02, _p(low), _p(high), 7, _p(out),
                                                 out.stride(0), _stream(h)), "f110_ddpg_actor_explore")
        elif mode == "env_gauss":
            actor_explore_env(h, W, b, scale, shift, s_in, s_out, 0.9995, 0.02, low, high, 7, out, kind=0)
        else:
            actor_explore_env(h, W, b, scale, shift, s_in, s_out, 0.9995, 0.02, low, high, 7, out, kind=1, ou_x=ou_x,
                              reset=rs, eval_mask=ev)

    def many(mode):
        for k in range(args.launches):
            launch(mode, k)

    graphs = {}
    side = torch.cuda.Stream(dev)
    for m in MODES:  # warm up, then capture
        many(m)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            many(m)
        graphs[m] = gr
    us = {m: {"eager": [], "graph": []} for m in MODES}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for m in MODES:
            for how, fn in (("eager", lambda: many(m)), ("graph", graphs[m].replay)):
                fn()  # this mode's code and data warm
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                us[m][how].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    res = {"rows": B, "hidden": K, "nout": n, "launches": args.launches, "rounds": args.rounds}
    for m in MODES:
        res[m] = {how: {"us_per_launch": [round(x, 3) for x in v], "median_us": float(np.median(v))}
                  for how, v in us[m].items()}
    for how in ("eager", "graph"):
        res[f"ou_masks_minus_explore_{how}_us"] = res["env_ou_masks"][how]["median_us"] - res["explore"][how]["median_us"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
