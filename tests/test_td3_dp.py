"""Data-parallel TD3 learner on CPU: two gloo ranks with half a batch each end every update with
the weights of one process on the whole batch (test_ddpg_dp.py's structure; the twin critics are one
gradient bucket, so a TD3 update that is no actor step is one all-reduce and an actor step two)."""
import os
import socket

import numpy as np
import torch

from conftest import golden


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _learner():
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    return DDPGLearner(obs_dim=12, act_dim=2, action_low=[-0.4189, 0.0], action_high=[0.4189, 20.0], seed=42,
                       device="cpu", replay=None, algo="td3", policy_delay=2)


def _batches():
    d = golden("ddpg.npz")
    S, A, R, S2, D = (torch.from_numpy(np.asarray(d[k])) for k in ("S", "A", "R", "S2", "D"))
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(4):
        idx = torch.randperm(S.shape[0], generator=g)[:32]
        w = torch.rand(32, generator=g)
        n = torch.randn(32, 2, generator=g)  # the smoothing draws, fixed: each rank takes its rows
        out.append((S[idx], A[idx], R[idx], S2[idx], D[idx].float(), w, n))
    return out


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from f110_gymnasium_ros2_jazzy_amd import distributed as D
    D.init(backend="gloo")
    ln = _learner()
    half = 32 // world
    for b in _batches():
        *rows, n = (t[rank * half:(rank + 1) * half] for t in b)
        ln.update(*rows, smooth_normals=n)
    nets = (ln.actor, ln.critic, ln.critic_target)
    q.put((rank, [{k: v.numpy().copy() for k, v in net.state_dict().items()} for net in nets]))  # numpy: no fd sharing
    D.shutdown()


def test_gloo_world2_matches_single_process_td3_update():
    import multiprocessing as mp
    torch.set_num_threads(1)
    ref = _learner()
    for b in _batches():
        ref.update(*b[:6], smooth_normals=b[6])
    assert ref.global_step == 4 and ref._last_actor_loss is not None  # updates 1 and 3 were actor steps
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=180) for _ in ps), key=lambda r: r[0])
    for p in ps:
        p.join(timeout=60)
    for _, nets in res:
        for got, net in zip(nets, (ref.actor, ref.critic, ref.critic_target)):
            for k, v in net.state_dict().items():
                np.testing.assert_allclose(got[k], v.numpy(), rtol=1e-5, atol=1e-7, err_msg=k)
    assert sorted({k.split(".")[0] for k in res[0][1][1]}) == ["c1", "c2"]
    for a, b in zip(res[0][1], res[1][1]):  # the ranks hold identical weights
        for k in a:
            assert np.array_equal(a[k], b[k])
