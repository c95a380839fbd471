"""Golden fixture for the per-row OU exploration head (f110_ddpg_actor_explore_env, kind 1).

TEST INFRASTRUCTURE ONLY.  Needs a checkout of the reference (F110_REFERENCE_ROOT, as
make_golden_ddpg.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ou.py

Executes the reference's own class, loaded by file path (no copy, make_golden_ddpg.load_ddpg):
  rl_training/DDPG/agent.py  OUActionNoise :469-505
one instance per row (the class keeps one state vector of act_dim entries), its `rng` replaced by
a recorded stream of float32 normals (the class casts its draw to float32, :497, so the recorded
value is the draw it uses), and records inputs and outputs only:

  ou_noise.npz  per scenario S in {A, B}:
    S_act      [calls][rows][nout] f32   the deterministic actions handed to __call__
    S_normals  [calls][rows][nout] f32   the draws
    S_reset    [calls][rows] u8          rows whose noise.reset() runs before the call
    S_low, S_high [nout] f32             the action box
    S_hyper    f64 [6]                   theta, mu, dt, sigma_start, sigma_min, decay
    S_out      [calls][rows][nout] f32   the returned actions (cast to the action's float32)
    S_x        [calls][rows][nout] f64   the state after every call
    S_sigma    [calls + 1] f64           sigma before every call, and after the last

  A: 5 rows x 2 outputs, the trainer's box [-0.4189, 0] .. [0.4189, 20], 40 calls, sigma 0.2
     decaying by 0.9 to the floor 0.05, rows 1 and 3 reset before call 10;
     the actions are spread past the box so that 64 of the 400 outputs sit on a bound (the
     script prints the count).
  B: 3 rows x 3 outputs, 12 calls, dt = 0.01 (an inexact sqrt), theta 0.3, row 2 reset before
     call 5.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ddpg import load_ddpg  # noqa: E402


class RecordedNormals:
    """Stands in for the class's np.random.Generator: normal(size=...) hands out the next recorded
    float32 draws (as float64, which the class casts back to the same float32)."""

    def __init__(self, draws):
        self.draws, self.i = np.asarray(draws, np.float32), 0

    def normal(self, size):
        d = self.draws[self.i]
        self.i += 1
        assert d.shape == tuple(size)
        return d.astype(np.float64)


def scenario(agm, name, rows, nout, calls, low, high, theta, mu, dt, sigma, sigma_min, decay, resets, spread, seed):
    rng = np.random.default_rng(seed)
    low, high = np.asarray(low, np.float32), np.asarray(high, np.float32)
    mid, half = 0.5 * (high + low), 0.5 * (high - low)
    act = (mid + half * rng.uniform(-spread, spread, (calls, rows, nout))).astype(np.float32)
    normals = rng.standard_normal((calls, rows, nout)).astype(np.float32)
    reset = np.zeros((calls, rows), np.uint8)
    for c, r in resets:
        reset[c, r] = 1
    noises = [agm.OUActionNoise(low, high, mu=mu, theta=theta, sigma_start=sigma, sigma_min=sigma_min, dt=dt,
                                decay=decay, seed=0) for _ in range(rows)]
    for r, nz in enumerate(noises):
        nz.rng = RecordedNormals(normals[:, r])
    out = np.zeros((calls, rows, nout), np.float32)
    x = np.zeros((calls, rows, nout), np.float64)
    sig = np.zeros(calls + 1, np.float64)
    for c in range(calls):
        sig[c] = noises[0].sigma
        for r, nz in enumerate(noises):
            if reset[c, r]:
                nz.reset()
            a = nz(torch.from_numpy(act[c, r].copy()), training=True)
            assert a.dtype == torch.float32
            out[c, r] = a.numpy()
            x[c, r] = nz.x
            assert nz.sigma == noises[0].sigma or r > 0
    sig[calls] = noises[0].sigma
    on_bound = int(((out == low) | (out == high)).sum())
    print(f"scenario {name}: {out.size} outputs, {on_bound} on a bound")
    hyper = np.array([theta, mu, dt, sigma, sigma_min, decay], np.float64)
    return {f"{name}_act": act, f"{name}_normals": normals, f"{name}_reset": reset, f"{name}_low": low,
            f"{name}_high": high, f"{name}_hyper": hyper, f"{name}_out": out, f"{name}_x": x, f"{name}_sigma": sig}


def main():
    _, agm = load_ddpg()
    arrays = {}
    arrays.update(scenario(agm, "A", rows=5, nout=2, calls=40, low=[-0.4189, 0.0], high=[0.4189, 20.0], theta=0.15,
                           mu=0.0, dt=1.0, sigma=0.2, sigma_min=0.05, decay=0.9, resets=[(10, 1), (10, 3)],
                           spread=1.15, seed=121))
    arrays.update(scenario(agm, "B", rows=3, nout=3, calls=12, low=[-1.0, -2.0, 0.0], high=[1.0, 2.0, 5.0],
                           theta=0.3, mu=0.0, dt=0.01, sigma=0.5, sigma_min=0.3, decay=0.95, resets=[(5, 2)],
                           spread=1.1, seed=202))
    path = os.path.join(HERE, "ou_noise.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote ou_noise.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
