"""TD3 on the device: the two TD3 heads (csrc/f110_td3.hip) against torch and against the host
hooks that run the same row rules, the smoothing head's own draw stream, the explicit TD3 update
against autograd and against the explicit DDPG update it reduces to, and the learner's / trainer's
HIP graphs (one capture set per update kind) against the eager loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOW2, HIGH2 = [-0.4189, 0.0], [0.4189, 20.0]


def _close(x, y, what):
    """test_gpu_ddpg_heads.py's rule: fp32 rounding of a reordered sum, a few ulps of the tensor's scale."""
    x, y = x.detach().cpu().numpy(), y.detach().cpu().numpy()
    np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-5 * float(np.abs(y).max()) + 1e-9, err_msg=what)


@pytest.mark.parametrize("B,K", [(1, 128), (7, 128), (9, 128), (333, 128), (64, 130), (40, 12)])
def test_critic_step_matches_torch(gpu, B, K):
    """f110_td3_critic_step: a partial last block (8 rows per block), several blocks, the non-float4
    K path and K below a half-wave's span, against the rule written out in torch float64."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import td3_critic_step
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + K)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    hs = [torch.relu(rn(B, K)) for _ in range(4)]  # ht1, ht2, h1, h2 (post-ReLU: zeros for the masks)
    Ws = [rn(1, K) * 0.2 for _ in range(4)]
    bs = [rn(1) * 0.1 for _ in range(4)]
    r, w = rn(B), torch.rand(B, device="cuda", generator=g) + 0.5
    d = (torch.rand(B, device="cuda", generator=g) < 0.3).float()
    gl = torch.full((), 0.7, device="cuda")
    out = td3_critic_step(hs[0], Ws[0], bs[0], hs[1], Ws[1], bs[1], r, d, 0.99, hs[2], Ws[2], bs[2], hs[3], Ws[3],
                          bs[3], w, gl, dh_masks=(hs[2], hs[3]))
    q = [(h.double() @ W.double().t() + b.double()).reshape(-1) for h, W, b in zip(hs, Ws, bs)]
    y = r.double() + 0.99 * (1.0 - d.double()) * torch.minimum(q[0], q[1])
    td1, td2 = y - q[2], y - q[3]
    if B >= 40:  # either target critic is the smaller one somewhere
        assert bool((q[0] < q[1]).any()) and bool((q[0] > q[1]).any())
    _close(out["td"].reshape(-1), (0.5 * (td1.abs() + td2.abs())).float(), "td")
    wd = w.double()
    for i, (td, h, W) in enumerate(((td1, hs[2], Ws[2]), (td2, hs[3], Ws[3])), 1):
        dq = -((0.7 / B) * wd) * (2.0 * td)
        _close(out[f"dq{i}"].reshape(-1), dq.float(), f"dq{i}")
        dh = (dq[:, None] * W.double()) * (h > 0)
        _close(out[f"dh{i}"], dh.float(), f"dh{i}")
        assert bool((out[f"dh{i}"][h <= 0] == 0).all())
    loss = (wd * td1 ** 2).mean() + (wd * td2 ** 2).mean()
    _close(out["part"].sum().reshape(1) / B, loss.float().reshape(1), "loss")


def _box(nout):
    low = torch.tensor((LOW2 + [-1.0])[:nout], device="cuda")
    high = torch.tensor((HIGH2 + [1.0])[:nout], device="cuda")
    return low, high, 0.5 * (high - low), 0.5 * (high + low)


@pytest.mark.parametrize("B", [1, 9, 333])
@pytest.mark.parametrize("nout", [1, 2, 3])
def test_target_action_matches_host_rule(gpu, B, nout):
    """f110_td3_target_action with caller-supplied draws: f110_ddpg_actor_head's action through the
    host hook (the same td3_smooth_one), bit for bit."""
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import _p, _stream, host_td3_smooth_rows, td3_target_action
    g = torch.Generator(device="cuda").manual_seed(B * 10 + nout)
    K = 128
    h = torch.relu(torch.randn(B, K, device="cuda", generator=g))
    W = torch.randn(nout, K, device="cuda", generator=g) * 0.2
    b = torch.randn(nout, device="cuda", generator=g) * 0.1
    n = torch.randn(B, nout, device="cuda", generator=g) * 2.0  # |0.2 n| > 0.5 on a good share of the draws
    low, high, scale, shift = _box(nout)
    act, t = torch.empty(B, nout, device="cuda"), torch.empty(B, nout, device="cuda")
    _lib.check(_lib.load().f110_ddpg_actor_head(_p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, nout, _p(act), _p(t),
                                                _stream(h)), "f110_ddpg_actor_head")
    out = td3_target_action(h, W, b, scale, shift, 0.2, 0.5, low, high, normals_ext=n)
    ref = host_td3_smooth_rows(act.cpu().numpy(), n.cpu().numpy(), 0.2, 0.5, scale.cpu().numpy(), low.cpu().numpy(),
                               high.cpu().numpy())
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    out0 = td3_target_action(h, W, b, scale, shift, 0.0, 0.5, low, high, normals_ext=n)  # no noise: clip(act)
    assert torch.equal(out0, torch.minimum(torch.maximum(act, low), high))


def test_target_action_device_draws(gpu):
    """normals_ext = NULL: with zero W / b, shift 0, scale 1, policy_noise 1 and both clips wide open
    the output is the draw itself.  65536 x 2 draws: mean / std / cross-correlation within
    test_actor_explore_head's bounds; the same (seed, counter) repeats, counter + 1 draws anew, and the
    stream is not f110_ddpg_actor_explore's for the same seed and counter."""
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import _p, _stream, td3_target_action
    M, K, seed = 65536, 128, 12345
    h = torch.zeros(M, K, device="cuda")
    W, b = torch.zeros(2, K, device="cuda"), torch.zeros(2, device="cuda")
    one, zero = torch.ones(2, device="cuda"), torch.zeros(2, device="cuda")
    lo, hi = torch.full((2,), -1e9, device="cuda"), torch.full((2,), 1e9, device="cuda")
    ctr = torch.tensor([5, 0], dtype=torch.int64, device="cuda")

    def draw():
        return td3_target_action(h, W, b, one, zero, 1.0, 1e9, lo, hi, seed=seed, counter=ctr)
    n1, n1b = draw(), draw()
    assert torch.equal(n1, n1b) and ctr.tolist() == [5, 0]  # the counter is only read
    ctr[0] = 6
    n2 = draw()
    assert float((n1 == n2).float().mean()) < 1e-3
    n = n1.double()
    se = 1.0 / M ** 0.5
    assert float(n.mean(0).abs().max()) < 4 * se
    assert float((n.std(0) - 1.0).abs().max()) < 4 * se * 0.75 + 0.01
    assert abs(float((n[:, 0] * n[:, 1]).mean())) < 4 * se
    # the exploration head's draws for the same seed and call index 5: sigma 1 on the same zero head
    st_in = torch.tensor([1.0, 5.0], dtype=torch.float64, device="cuda")
    st_out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ex = torch.empty(M, 2, device="cuda")
    _lib.check(_lib.load().f110_ddpg_actor_explore(_p(h), _p(W), _p(b), _p(one), _p(zero), M, K, 2, _p(st_in),
                                                   _p(st_out), 1.0, 0.0, _p(lo), _p(hi), seed, _p(ex), 2, _stream(h)),
               "f110_ddpg_actor_explore")
    assert float((ex == n1).float().mean()) < 1e-3
    assert abs(float(ex.double().std()) - 1.0) < 0.02  # (it did draw)


def _data(M, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    S = torch.randn(M, D, device="cuda", generator=g)
    A = torch.rand(M, 2, device="cuda", generator=g) * torch.tensor([0.8378, 20.0], device="cuda") - \
        torch.tensor([0.4189, 0.0], device="cuda")
    R = torch.randn(M, device="cuda", generator=g)
    S2 = S + 0.1 * torch.randn(M, D, device="cuda", generator=g)
    Dn = (torch.rand(M, device="cuda", generator=g) < 0.1).float()
    W = torch.rand(M, device="cuda", generator=g) + 0.5
    N = [torch.randn(M, 2, device="cuda", generator=g) for _ in range(3)]
    return (S, A, R, S2, Dn, W), N


def _learner(D, algo="td3", **kw):
    import f110_gymnasium_ros2_jazzy_amd.ddpg as Dd
    return Dd.DDPGLearner(obs_dim=D, act_dim=2, action_low=LOW2, action_high=HIGH2, seed=1, device="cuda:0",
                          replay=None, algo=algo, **kw)


def _bucket_close(x, y):
    tol = 1e-4 * y.abs() + 1e-5 * y.abs().max()
    assert bool(((x - y).abs() <= tol).all()), float(((x - y).abs() / tol).max())


@pytest.mark.parametrize("M,D", [(333, 64), (64, 12)])
def test_explicit_td3_matches_autograd(gpu, monkeypatch, M, D):
    """ExplicitUpdate.critic with twin critics / actor(cr=c1) against the autograd TD3 learner on the same
    weights, batch and smoothing draws, policy_delay 2, three updates (critic-only, actor step, critic-only):
    test_explicit_update_matches_autograd's tolerances."""
    import f110_gymnasium_ros2_jazzy_amd.ddpg as Dd
    batch, N = _data(M, D, M + D)
    runs = []
    for explicit in (True, False):
        monkeypatch.setattr(Dd, "EXPLICIT", explicit)
        ln = _learner(D, policy_delay=2)
        assert (ln.explicit is not None) == explicit
        st = ln.update(*batch, smooth_normals=N[0])
        assert st["actor_loss"] is None
        closs = [float(st["critic_loss"])]
        grads = [ln.critic_grads.flat.clone(), st["td"].clone()]
        st = ln.update(*batch, smooth_normals=N[1])
        closs.append(float(st["critic_loss"]))
        aloss = float(st["actor_loss"])
        grads.append(ln.actor_grads.flat.clone())
        pol = ln.choose_action(batch[0][:100], training=False).clone()
        st = ln.update(*batch, smooth_normals=N[2])
        closs.append(float(st["critic_loss"]))
        assert float(st["actor_loss"]) == aloss  # no actor step: the last one's loss
        runs.append((closs + [aloss], grads, pol))
    np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=1e-4)
    for x, y in zip(runs[0][1], runs[1][1]):
        _bucket_close(x, y)
    torch.testing.assert_close(runs[0][2], runs[1][2], rtol=1e-5, atol=1e-6)


def test_explicit_td3_reduces_to_ddpg(gpu):
    """Equal critics, policy_noise 0, policy_delay 1 on the explicit path: the actor and c1 follow the
    explicit DDPG learner (each critic's gradient of the summed loss is DDPG's; min(q, q) = q)."""
    M, D = 333, 64
    batch, _ = _data(M, D, 5)
    t, dd = _learner(D, policy_noise=0.0, policy_delay=1), _learner(D, "ddpg")
    assert t.explicit is not None and dd.explicit is not None
    t.critic.c2.load_state_dict(t.critic.c1.state_dict())
    t.critic_target.c2.load_state_dict(t.critic_target.c1.state_dict())
    n1 = dd.critic_grads.flat.numel()
    assert t.critic_grads.flat.numel() == 2 * n1
    losses = [[], []]
    for k in range(3):
        st, sd = t.update(*batch), dd.update(*batch)
        losses[0].append((0.5 * float(st["critic_loss"]), float(st["actor_loss"])))
        losses[1].append((float(sd["critic_loss"]), float(sd["actor_loss"])))
        if k == 0:
            _bucket_close(t.critic_grads.flat[:n1], dd.critic_grads.flat)
            _bucket_close(t.critic_grads.flat[n1:], dd.critic_grads.flat)
            _bucket_close(t.actor_grads.flat, dd.actor_grads.flat)
            _bucket_close(st["td"], sd["td"].abs())
            pol = (t.choose_action(batch[0][:100], training=False).clone(),
                   dd.choose_action(batch[0][:100], training=False).clone())
    np.testing.assert_allclose(losses[0], losses[1], rtol=1e-4)
    torch.testing.assert_close(pol[0], pol[1], rtol=1e-5, atol=1e-6)


def test_td3_learner_graphs_match_eager(gpu):
    """replay() as HIP-graph replays for TD3 (one capture set per update kind, picked by global_step)
    follows the eager learner: test_learner_graphs_match_eager's data and tolerances."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    g = torch.Generator(device="cuda").manual_seed(5)
    D = 64
    S = torch.randn(512, D, device="cuda", generator=g)
    A = torch.rand(512, 2, device="cuda", generator=g) * torch.tensor([0.8378, 20.0], device="cuda") - \
        torch.tensor([0.4189, 0.0], device="cuda")
    R = torch.randn(512, device="cuda", generator=g)
    S2 = S + 0.1 * torch.randn(512, D, device="cuda", generator=g)
    Dn = torch.rand(512, device="cuda", generator=g) < 0.1
    runs = []
    for graphs in (False, True):
        ln = DDPGLearner(obs_dim=D, act_dim=2, action_low=LOW2, action_high=HIGH2, seed=3, device="cuda:0",
                         memory_size=1024, batch_size=128, graphs=graphs, algo="td3", policy_delay=2)
        ln.remember(S, A, R, S2, Dn)
        losses = []
        for k in range(8):
            st = ln.replay()
            assert (st["actor_loss"] is None) == (k == 0)
            losses.append((float(st["critic_loss"]), float(st["actor_loss"]) if k else 0.0))
        if graphs:
            assert sorted(ln._graphs) == [False, True] and [len(v) for _, v in sorted(ln._graphs.items())] == [2, 3]
        assert ln.global_step == 8 and int(ln.critic_optim.state[0]) == 8 and int(ln.actor_optim.state[0]) == 4
        runs.append((losses, [p.detach().clone() for p in list(ln.actor.parameters()) + list(ln.critic.parameters())],
                     ln.memory.priorities().clone()))
        ln.memory.close()
    np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=1e-4)
    for a, b in zip(runs[0][1], runs[1][1]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(runs[0][2], runs[1][2], rtol=1e-3, atol=1e-6)


def test_td3_trainer_step_graphs_match_eager(gpu, monkeypatch):
    """VectorTrainer's whole-step graphs with algo td3 (captures per parity and update kind) against
    the eager loop (F110_STEP_GRAPH=0): weights, ring, noise state and losses bit-identical after 14
    steps, losses also after 13 (test_trainer_step_graphs_match_eager's checks)."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    runs, l13 = [], []
    for flag in ("1", "0"):
        monkeypatch.setenv("F110_STEP_GRAPH", flag)
        tr = VectorTrainer(256, batch_size=256, memory_size=4096, warmup_steps=3, seed=11, algo="td3")
        for _ in range(13):
            tr.step()
        l13.append((float(tr.last["critic_loss"]), float(tr.last["actor_loss"])))
        tr.step()
        torch.cuda.synchronize()
        # updates 0-2 are the eager warm-up; then step parity and update kind alternate together
        captured = [k in tr._sg for k in ((0, True), (1, True), (0, False), (1, False))]  # (parity, actor step)
        assert captured == ([True, False, False, True] if flag == "1" else [False] * 4)
        ag = tr.agent
        params = [p.detach().clone() for p in list(ag.actor.parameters()) + list(ag.critic.parameters()) +
                  list(ag.actor_target.parameters()) + list(ag.critic_target.parameters())]
        n = len(ag.memory)
        ring = {k: v[:n].clone() for k, v in ag.memory.arrays().items()}
        runs.append((params, ring, float(tr.last["critic_loss"]), float(tr.last["actor_loss"]), ag.sigma,
                     ag._noise_calls, tr.obs.clone(), len(ag.memory), ag.global_step))
        tr.close()
    (pa, ra, ca, aa, sa, na, oa, la, ga), (pb, rb_, cb, ab, sb, nb, ob, lb, gb) = runs
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    for k in ra:
        assert torch.equal(ra[k], rb_[k]), k
    assert (ca, aa, sa, na, la, ga) == (cb, ab, sb, nb, lb, gb) and ga == 11
    assert torch.equal(oa, ob)
    assert l13[0] == l13[1]


def test_td3_trainer_loop(gpu):
    """30 steps of the trainer with algo td3, 3-step returns and OU noise: finite losses and weights,
    the learner counts updates, the actor's optimizer stepped on every policy_delay-th of them."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    tr = VectorTrainer(256, batch_size=256, memory_size=4096, warmup_steps=5, seed=3, algo="td3", n_step=3,
                       noise_type="ou")
    for _ in range(30):
        tr.step()
    torch.cuda.synchronize()
    st, ag = tr.last, tr.agent
    assert st is not None and torch.isfinite(st["critic_loss"]) and torch.isfinite(st["actor_loss"])
    assert ag.global_step == 25 and ag.policy_delay == 2
    assert int(ag.actor_optim.state[0]) == ag.global_step // ag.policy_delay == 12
    assert int(ag.critic_optim.state[0]) == 25
    for p in list(ag.actor.parameters()) + list(ag.critic.parameters()) + list(ag.critic_target.parameters()):
        assert torch.isfinite(p).all()
    tr.close()
