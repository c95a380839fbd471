"""TD3, host side (no GPU): the two row rules the TD3 kernels run (td3_smooth_one / td3_row through
f110_host_td3_smooth_rows / f110_host_td3_rows) against NumPy float32 restatements bit for bit, the
new entry points' validation (refused before any device call), and the CPU learner: seed order,
the delayed-update schedule, the reduction to DDPG, the clipped double-Q target and checkpoints."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

LOW2, HIGH2 = [-0.4189, 0.0], [0.4189, 20.0]  # the trainer's action box
F32 = np.float32


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def H():
    from f110_gymnasium_ros2_jazzy_amd import ddpg_heads
    return ddpg_heads


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_exports(F):
    L = F.load()
    for n in ("f110_td3_target_action", "f110_td3_critic_step", "f110_host_td3_smooth_rows", "f110_host_td3_rows"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION


# ---- td3_smooth_one ------------------------------------------------------------------------------
def smooth_model(act, n, pn, nc, scale, lo, hi):
    """td3_smooth_one in NumPy float32 (IEEE single, no FMA), with the four clip counts."""
    s = F32(pn) * scale
    c = F32(nc) * scale
    e = s * n
    below, above = e < -c, e > c
    e = np.where(below, -c, e)
    e = np.where(e > c, c, e)
    v = act + e
    at_lo = v < lo
    v = np.where(at_lo, lo, v)
    at_hi = v > hi
    v = np.where(at_hi, hi, v)
    return v.astype(F32), (int(below.sum()), int(above.sum()), int(at_lo.sum()), int(at_hi.sum()))


def _box(nout):
    low = np.array((LOW2 + [-1.0])[:nout], F32)
    high = np.array((HIGH2 + [1.0])[:nout], F32)
    return low, high, (F32(0.5) * (high - low)).astype(F32)


@pytest.mark.parametrize("nout", [1, 2, 3])
def test_smooth_rows_match_numpy_bit_for_bit(H, nout):
    rng = np.random.default_rng(100 + nout)
    low, high, scale = _box(nout)
    act = (low + rng.random((4096, nout), dtype=F32) * (high - low)).astype(F32)  # anywhere in the box: edges are hit
    n = rng.standard_normal((4096, nout), dtype=F32)  # |n| > 2.5 hits the noise clip (0.5 / 0.2)
    ref, counts = smooth_model(act, n, 0.2, 0.5, scale, low, high)
    assert all(c > 0 for c in counts), counts  # each side of the noise clip and of the box
    out = H.host_td3_smooth_rows(act, n, 0.2, 0.5, scale, low, high)
    assert np.array_equal(bits(out), bits(ref))
    # a clip left out would show: the unclipped noise / the unclipped sum differ from the model somewhere
    assert not np.array_equal(ref, np.clip(act + F32(0.2) * scale * n, low, high))
    assert not np.array_equal(ref, act + np.clip(F32(0.2) * scale * n, -F32(0.5) * scale, F32(0.5) * scale))


def test_smooth_rows_nan_and_zero_noise(H):
    low, high, scale = _box(2)
    act = np.array([[np.nan, 3.0], [0.1, np.nan], [0.5, 25.0], [-0.7, -1.0]], F32)
    n = np.ones((4, 2), F32)
    out = H.host_td3_smooth_rows(act, n, 0.2, 0.5, scale, low, high)
    assert np.isnan(out[0, 0]) and np.isnan(out[1, 1]) and not np.isnan(out[0, 1]) and not np.isnan(out[1, 0])
    out0 = H.host_td3_smooth_rows(act, n * 7, 0.0, 0.5, scale, low, high)  # policy_noise = 0: clip(act)
    want = np.clip(act, low, high)
    assert np.array_equal(bits(out0[2:]), bits(want[2:])) and out0[2, 1] == 20.0 and out0[3, 0] == low[0]
    assert np.isnan(out0[0, 0]) and out0[0, 1] == 3.0


# ---- td3_row -------------------------------------------------------------------------------------
def rows_model(r, d, gamma, q1t, q2t, q1, q2, w, g, B):
    with np.errstate(invalid="ignore"):
        m = np.where((q2t < q1t) | (q2t != q2t), q2t, q1t)
        y = r + (F32(gamma) * (F32(1.0) - d)) * m
        td1, td2 = y - q1, y - q2
        gb = F32(g) / F32(B)
        dq1 = -((gb * w) * (F32(2.0) * td1))
        dq2 = -((gb * w) * (F32(2.0) * td2))
        prio = F32(0.5) * (np.abs(td1) + np.abs(td2))
        wl = w * (td1 * td1) + w * (td2 * td2)
    return dict(td1=td1, td2=td2, dq1=dq1, dq2=dq2, prio=prio, wl=wl)


def test_twin_rows_match_numpy_bit_for_bit(H):
    B = 1000
    rng = np.random.default_rng(7)
    r, q1t, q2t, q1, q2 = (rng.standard_normal(B, dtype=F32) * F32(3.0) for _ in range(5))
    w = (rng.random(B, dtype=F32) + F32(0.5)).astype(F32)
    d = (rng.random(B) < 0.1).astype(F32)
    q2t[:50] = q1t[:50]           # ties
    q1t[60], q2t[61] = np.nan, np.nan
    d[70] = 1.0
    assert (q1t < q2t).any() and (q1t > q2t).any() and (q1t == q2t).sum() >= 50 and (d == 1).any()
    assert np.isnan(q1t).sum() == 1 and np.isnan(q2t).sum() == 1
    ref = rows_model(r, d, 0.99, q1t, q2t, q1, q2, w, 1.0, B)
    out = H.host_td3_rows(r, d, 0.99, q1t, q2t, q1, q2, w, 1.0)
    # torch.minimum's NaN propagation, from either side, and only there
    nan_rows = np.isnan(out["td1"])
    assert nan_rows[60] and nan_rows[61] and nan_rows.sum() == 2
    ok = ~nan_rows
    for k in ("td1", "td2", "dq1", "dq2", "prio", "wl"):  # (a NaN's sign and payload are not part of the rule)
        assert np.array_equal(bits(out[k][ok]), bits(ref[k][ok])), k
        assert np.isnan(out[k][nan_rows]).all() and np.isnan(ref[k][nan_rows]).all(), k
    assert (out["prio"][ok] >= 0).all()
    y64 = r.astype(np.float64) + 0.99 * (1.0 - d) * np.minimum(q1t, q2t).astype(np.float64)
    np.testing.assert_allclose(out["td1"][ok], (y64 - q1)[ok], rtol=1e-5, atol=1e-5)
    done = (d == 1) & ok  # a done row bootstraps nothing (0 * NaN is still NaN, as in torch)
    assert done.any() and np.array_equal(out["td1"][done], (r - q1)[done])


# ---- validation: refused before any device call ---------------------------------------------------
def _P(v):
    return ctypes.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v


def _target_action(F, **over):
    """Host memory stands in for the device buffers: the validation runs before the first device
    call, so nothing is dereferenced."""
    B, K, nout = 4, 8, 2
    f = lambda *s: np.zeros(s, F32)  # noqa: E731
    a = dict(h=f(B, K), W=f(nout, K), b=f(nout), scale=f(nout), shift=f(nout), B=B, K=K, nout=nout, policy_noise=0.2,
             noise_clip=0.5, low=f(nout), high=f(nout), seed=1, counter=np.zeros(2, np.int64), normals_ext=None,
             out=f(B, nout))
    a.update(over)
    L = F.load()
    rc = L.f110_td3_target_action(*[_P(a[k]) for k in (
        "h", "W", "b", "scale", "shift", "B", "K", "nout", "policy_noise", "noise_clip", "low", "high", "seed",
        "counter", "normals_ext", "out")], None)
    return rc, (L.f110_last_error() or b"").decode()


@pytest.mark.parametrize("over", [
    dict(h=None), dict(W=None), dict(b=None), dict(scale=None), dict(shift=None), dict(low=None), dict(high=None),
    dict(out=None), dict(B=0), dict(B=-3), dict(K=256), dict(nout=5), dict(policy_noise=-0.1),
    dict(policy_noise=float("nan")), dict(policy_noise=float("inf")), dict(noise_clip=-1.0),
    dict(noise_clip=float("nan")), dict(noise_clip=float("inf")), dict(counter=None),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_target_action_refuses_bad_arguments(F, over):
    rc, msg = _target_action(F, **over)
    assert rc == -1 and "f110_td3_target_action" in msg


_CS = ("ht1", "Wt1", "bt1", "ht2", "Wt2", "bt2", "r", "d", "gamma", "h1", "W1", "b1", "h2", "W2", "b2", "w", "g", "B",
       "K", "td", "dh1", "dh1_mask", "dh2", "dh2_mask", "dq1", "dq2", "part")


def _critic_step(F, **over):
    B, K = 4, 8
    f = lambda *s: np.zeros(s, F32)  # noqa: E731
    a = {k: f(B, K) for k in ("ht1", "ht2", "h1", "h2", "dh1", "dh2")}
    a.update({k: f(1, K) for k in ("Wt1", "Wt2", "W1", "W2")})
    a.update({k: f(1) for k in ("bt1", "bt2", "b1", "b2", "g", "part")})
    a.update({k: f(B) for k in ("r", "d", "w", "td", "dq1", "dq2")})
    a.update(gamma=0.99, B=B, K=K, dh1_mask=None, dh2_mask=None)
    a.update(over)
    L = F.load()
    rc = L.f110_td3_critic_step(*[_P(a[k]) for k in _CS], None)
    return rc, (L.f110_last_error() or b"").decode()


@pytest.mark.parametrize("over", [dict([(k, None)]) for k in (
    "ht1", "Wt1", "bt1", "ht2", "Wt2", "bt2", "r", "d", "h1", "W1", "b1", "h2", "W2", "b2", "w", "g", "td", "part")] +
    [dict(B=0), dict(B=-1), dict(K=256), dict(K=0)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_critic_step_refuses_bad_arguments(F, over):
    rc, msg = _critic_step(F, **over)
    assert rc == -1 and "f110_td3_critic_step" in msg


def test_host_hooks_refuse_bad_arguments(F):
    L = F.load()
    a = np.zeros((3, 2), F32)
    v = np.zeros(2, F32)

    def smooth(act=a, n=a, rows=3, nout=2, pn=0.2, nc=0.5, scale=v, low=v, high=v, out=a.copy()):
        return L.f110_host_td3_smooth_rows(_P(act), _P(n), rows, nout, pn, nc, _P(scale), _P(low), _P(high), _P(out))
    assert smooth() == 0
    for kw in (dict(act=None), dict(n=None), dict(scale=None), dict(low=None), dict(high=None), dict(out=None),
               dict(rows=0), dict(nout=5), dict(nout=0), dict(pn=-1.0), dict(pn=float("nan")), dict(nc=float("inf")),
               dict(nc=-0.5)):
        assert smooth(**kw) == -1, kw
        assert b"f110_host_td3_smooth_rows" in L.f110_last_error()
    x = np.zeros(3, F32)
    outs = [np.zeros(3, F32) for _ in range(6)]

    def rows(B=3, drop=None):
        ins = [x] * 7
        args = [_P(ins[0]), _P(ins[1]), 0.99] + [_P(t) for t in ins[2:]] + [1.0, B] + [_P(o) for o in outs]
        if drop is not None:
            args[drop] = None
        return L.f110_host_td3_rows(*args)
    assert rows() == 0
    assert rows(B=0) == -1 and rows(B=-2) == -1
    for i in (0, 1, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15):
        assert rows(drop=i) == -1, i
    assert b"f110_host_td3_rows" in L.f110_last_error()


# ---- the CPU learner -------------------------------------------------------------------------------
def _learner(algo="td3", seed=42, **kw):
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    return DDPGLearner(obs_dim=12, act_dim=2, action_low=LOW2, action_high=HIGH2, seed=seed, device="cpu",
                       replay=None, algo=algo, **kw)


@pytest.fixture(scope="module")
def batches():
    """Four batches of 32 drawn as test_ddpg_dp.py draws them, plus fixed smoothing draws."""
    d = golden("ddpg.npz")
    S, A, R, S2, D = (torch.from_numpy(np.asarray(d[k])) for k in ("S", "A", "R", "S2", "D"))
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(4):
        idx = torch.randperm(S.shape[0], generator=g)[:32]
        w = torch.rand(32, generator=g)
        out.append((S[idx], A[idx], R[idx], S2[idx], D[idx].float(), w))
    normals = [torch.randn(32, 2, generator=g) for _ in range(4)]
    return out, normals


def _sd(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_arguments_are_validated():
    for kw in (dict(algo="sac"), dict(policy_delay=0), dict(policy_delay=1.5), dict(policy_noise=-0.1),
               dict(policy_noise=float("nan")), dict(noise_clip=float("inf")), dict(noise_clip=-1.0)):
        with pytest.raises(ValueError):
            _learner(**kw)
    with pytest.raises(ValueError):  # checked for "ddpg" too, then unused
        _learner(algo="ddpg", policy_delay=0)


def test_seed_anchor():
    """The same seed gives TD3 the actor and first critic DDPG gets (c2 and its target are drawn last)."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg import TwinCritic
    t, dd = _learner("td3"), _learner("ddpg")
    assert isinstance(t.critic, TwinCritic) and isinstance(t.critic_target, TwinCritic)
    assert _same(_sd(t.actor), _sd(dd.actor)) and _same(_sd(t.critic.c1), _sd(dd.critic))
    assert _same(_sd(t.actor_target), _sd(dd.actor_target)) and _same(_sd(t.critic_target.c1), _sd(dd.critic_target))
    assert not torch.equal(t.critic.c2.fcs1.weight, t.critic.c1.fcs1.weight)
    assert _same(_sd(t.critic_target), _sd(t.critic))  # targets start as copies
    q1, q2 = t.critic(torch.zeros(3, 12), torch.zeros(3, 2))
    assert q1.shape == q2.shape == (3, 1)
    assert [k.split(".")[0] for k in t.critic.state_dict()] == ["c1"] * 6 + ["c2"] * 6


def test_delayed_update_schedule(batches):
    bs, normals = batches
    ln = _learner(policy_delay=3)
    a0, at0, ct0, c0 = _sd(ln.actor), _sd(ln.actor_target), _sd(ln.critic_target), _sd(ln.critic)
    for u in range(2):
        assert not ln.is_actor_step()
        st = ln.update(*bs[u], smooth_normals=normals[u])
        assert st["actor_loss"] is None and torch.isfinite(st["critic_loss"])
        assert st["td"].shape == (32, 1) and bool((st["td"] >= 0).all())
        assert _same(_sd(ln.actor), a0) and _same(_sd(ln.actor_target), at0) and _same(_sd(ln.critic_target), ct0)
        c = _sd(ln.critic)
        assert not torch.equal(c["c1.fcs1.weight"], c0["c1.fcs1.weight"])
        assert not torch.equal(c["c2.fcs1.weight"], c0["c2.fcs1.weight"])
        c0 = c
    assert ln.is_actor_step()
    st = ln.update(*bs[2], smooth_normals=normals[2])
    assert st["actor_loss"] is not None and torch.isfinite(st["actor_loss"])
    for now, before in ((ln.actor, a0), (ln.actor_target, at0), (ln.critic, c0)):
        assert not torch.equal(_sd(now)["fc1.weight" if "fc1.weight" in before else "c1.fcs1.weight"],
                               before["fc1.weight" if "fc1.weight" in before else "c1.fcs1.weight"])
    ct = _sd(ln.critic_target)
    assert not torch.equal(ct["c1.fcs1.weight"], ct0["c1.fcs1.weight"])
    assert not torch.equal(ct["c2.fcs1.weight"], ct0["c2.fcs1.weight"])
    last = st["actor_loss"]
    st = ln.update(*bs[3], smooth_normals=normals[3])  # no actor step: the last actor step's loss
    assert st["actor_loss"] is last and ln.global_step == 4


def test_reduces_to_ddpg(batches):
    """Equal critics, no smoothing noise, no delay: each critic's gradient of the summed loss is
    DDPG's and min(q, q) = q, so the actor, c1 and their targets follow a DDPG learner."""
    bs, _ = batches
    t, dd = _learner("td3", policy_noise=0.0, policy_delay=1), _learner("ddpg")
    t.critic.c2.load_state_dict(t.critic.c1.state_dict())
    t.critic_target.c2.load_state_dict(t.critic_target.c1.state_dict())
    for b in bs:
        st, sd = t.update(*b), dd.update(*b)
        np.testing.assert_allclose(float(st["critic_loss"]), 2.0 * float(sd["critic_loss"]), rtol=1e-5)
        np.testing.assert_allclose(float(st["actor_loss"]), float(sd["actor_loss"]), rtol=1e-5)
        np.testing.assert_allclose(st["td"].numpy(), sd["td"].abs().numpy(), rtol=1e-5, atol=1e-6)
    for got, ref in ((t.actor, dd.actor), (t.critic.c1, dd.critic), (t.actor_target, dd.actor_target),
                     (t.critic_target.c1, dd.critic_target)):
        for k, v in ref.state_dict().items():
            np.testing.assert_allclose(got.state_dict()[k].numpy(), v.numpy(), rtol=1e-6, atol=1e-7, err_msg=k)


def test_target_takes_the_minimum(batches):
    bs, normals = batches
    ln = _learner()
    with torch.no_grad():  # non-trivial heads (the reference inits them near 0), distinct critics
        g = torch.Generator().manual_seed(3)
        for c in (ln.critic_target.c1, ln.critic_target.c2):
            c.q.weight.copy_(torch.randn(c.q.weight.shape, generator=g) * 0.2)
            c.q.bias.copy_(torch.randn(1, generator=g) * 0.1)
    S, A, R, S2, D, W = bs[0]
    r, d = R.reshape(-1, 1), D.reshape(-1, 1)
    y = ln._td3_target(S2, r, d, normals[0])
    at, ct = copy.deepcopy(ln.actor_target).double(), copy.deepcopy(ln.critic_target).double()
    with torch.no_grad():
        lo, hi = torch.tensor(LOW2, dtype=torch.float64), torch.tensor(HIGH2, dtype=torch.float64)
        scale = 0.5 * (hi - lo)
        e = torch.clamp(0.2 * scale * normals[0].double(), -0.5 * scale, 0.5 * scale)
        a2 = torch.clamp(at(S2.double()) + e, lo, hi)
        q1t, q2t = ct(S2.double(), a2)
        y64 = r.double() + 0.99 * (1.0 - d.double()) * torch.minimum(q1t, q2t)
    assert bool((q1t < q2t).any()) and bool((q1t > q2t).any())  # either critic alone would miss
    np.testing.assert_allclose(y.numpy(), y64.numpy(), rtol=1e-6, atol=1e-6)
    assert float((y64 - (r.double() + 0.99 * (1.0 - d.double()) * q1t)).abs().max()) > 1e-4


def test_checkpoint_round_trip(batches, tmp_path):
    bs, normals = batches
    ln = _learner(policy_delay=2)
    ln.path = str(tmp_path)
    for u in range(3):
        ln.update(*bs[u], smooth_normals=normals[u])
    ln.save_model("td3.pt")
    ck = torch.load(tmp_path / "td3.pt", weights_only=True)
    assert (ck["algo"], ck["policy_delay"], ck["policy_noise"], ck["noise_clip"]) == ("td3", 2, 0.2, 0.5)
    assert sorted({k.split(".")[0] for k in ck["critic"]}) == ["c1", "c2"] == sorted(
        {k.split(".")[0] for k in ck["critic_target"]})
    assert len(ck["critic_optim"]["state"]) == 12
    other = _learner(seed=7, policy_delay=2)
    other.path = str(tmp_path)
    assert other.load_model("td3.pt")
    for a, b in ((other.actor, ln.actor), (other.critic, ln.critic), (other.actor_target, ln.actor_target),
                 (other.critic_target, ln.critic_target)):
        assert _same(_sd(a), _sd(b))
    assert other.global_step == 3 and other.is_actor_step() == ln.is_actor_step() is True
    st, so = ln.update(*bs[3], smooth_normals=normals[3]), other.update(*bs[3], smooth_normals=normals[3])
    assert torch.equal(st["critic_loss"], so["critic_loss"]) and _same(_sd(other.critic), _sd(ln.critic))
    assert _same(_sd(other.actor), _sd(ln.actor))
    # a DDPG checkpoint (no "algo" key) and a TD3 learner, and the reverse
    dd = _learner("ddpg")
    dd.path = str(tmp_path)
    dd.save_model("ddpg.pt")
    assert "algo" not in torch.load(tmp_path / "ddpg.pt", weights_only=True)
    with pytest.raises(ValueError, match="ddpg"):
        other.load_model("ddpg.pt")
    with pytest.raises(ValueError, match="td3"):
        dd.load_model("td3.pt")


@pytest.mark.parametrize("algo,want", [("ddpg", [["critic", "actor"]] * 4),
                                       ("td3", [["critic"], ["critic", "actor"]] * 2)])
def test_update_schedule_runs_through_the_phase_runner(batches, algo, want):
    """update() is the learner's phases under _run_phases: the critic bucket is reduced in every
    update, the actor bucket only in an actor step (every DDPG update, every second TD3 update with
    policy_delay 2), critic first.  A one-entry phase list is a whole update: nothing is reduced."""
    bs, normals = batches
    ln = _learner(algo, policy_delay=2)
    calls = []
    ln.critic_grads.reduce = lambda: calls.append("critic")
    ln.actor_grads.reduce = lambda: calls.append("actor")
    got = []
    for _ in range(4):
        del calls[:]
        ln.update(*bs[0], smooth_normals=normals[0])
        got.append(list(calls))
    assert got == want and ln.global_step == 4
    del calls[:]
    ln._run_phases([lambda: calls.append("whole")])
    assert calls == ["whole"]
