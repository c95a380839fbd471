"""The per-row exploration head, host side (no GPU): f110_host_explore_rows -- the function the
kExploreEnv epilogue of k_head_fwd runs, over host arrays -- against the reference's OUActionNoise
(tests/golden/ou_noise.npz, recorded by make_golden_ou.py) bit for bit, against a NumPy float32
restatement of GaussianActionNoise, on eval and reset rows, and f110_ddpg_actor_explore_env's
validation, which refuses a bad argument before any device call."""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ou_noise.npz")


@pytest.fixture(scope="module")
def F():
    from f110_gymnasium_ros2_jazzy_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def H():
    from f110_gymnasium_ros2_jazzy_amd import ddpg_heads
    return ddpg_heads


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_exports(F):
    L = F.load()
    for n in ("f110_ddpg_actor_explore_env", "f110_host_explore_rows"):
        assert n in F.EXPORTS and hasattr(L, n)
    assert L.f110_abi_version() == 3 == F.ABI_VERSION


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_golden_shape(G):
    assert G["A_act"].shape == (40, 5, 2) and G["B_act"].shape == (12, 3, 3)
    out = G["A_out"]
    assert int(((out == G["A_low"]) | (out == G["A_high"])).sum()) == 64  # the clip is exercised
    assert G["A_reset"][10].tolist() == [0, 1, 0, 1, 0] and G["A_reset"].sum() == 2
    assert G["A_sigma"][0] == 0.2 and G["A_sigma"][-1] == 0.05 and G["A_hyper"][1] == 0.0  # mu = 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_ou_matches_reference_bit_for_bit(H, G, name):
    act, nrm, rst = G[f"{name}_act"], G[f"{name}_normals"], G[f"{name}_reset"]
    theta, mu, dt, sigma, sigma_min, decay = G[f"{name}_hyper"].tolist()
    calls, rows, nout = act.shape
    x = np.zeros((rows, nout), np.float64)
    for c in range(calls):
        assert sigma == G[f"{name}_sigma"][c], c
        out, (sigma, call) = H.host_explore_rows(act[c], nrm[c], 1, x, sigma, G[f"{name}_low"], G[f"{name}_high"],
                                                 theta=theta, mu=mu, dt=dt, reset=rst[c], decay=decay,
                                                 sigma_min=sigma_min, call=c)
        assert call == c + 1
        assert np.array_equal(bits(x), bits(G[f"{name}_x"][c])), f"x, call {c}"
        assert np.array_equal(bits(out), bits(G[f"{name}_out"][c])), f"actions, call {c}"
    assert sigma == G[f"{name}_sigma"][calls]


def test_gaussian_matches_numpy_f32(H):
    rng = np.random.default_rng(3)
    low, high = np.array([-0.4189, 0.0, -1.0], np.float32), np.array([0.4189, 20.0, 1.0], np.float32)
    act = (rng.uniform(-1.2, 1.2, (37, 3)) * (high - low) / 2 + (high + low) / 2).astype(np.float32)
    act[5, 1] = np.nan
    nrm = rng.standard_normal((37, 3)).astype(np.float32)
    sigma = 0.2 * 0.9995 ** 3
    out, (s2, call) = H.host_explore_rows(act, nrm, 0, None, sigma, low, high, decay=0.9995, sigma_min=0.02, call=7)
    v = act + np.float32(sigma) * nrm  # float32 throughout, as kExplore
    assert v.dtype == np.float32
    v = np.where(v < low, low, v)
    v = np.where(v > high, high, v)
    assert np.array_equal(bits(out), bits(v))
    assert np.isnan(out[5, 1])
    assert ((out == low) | (out == high)).sum() > 5
    assert s2 == max(sigma * 0.9995, 0.02) and call == 8.0
    # the floor
    _, (s3, _) = H.host_explore_rows(act, nrm, 0, None, 0.0201, low, high, decay=0.9, sigma_min=0.02)
    assert s3 == 0.02


@pytest.mark.parametrize("kind", [0, 1])
def test_eval_and_reset_rows(H, kind):
    rng = np.random.default_rng(kind)
    low, high = np.array([-0.4189, 0.0], np.float32), np.array([0.4189, 20.0], np.float32)
    act = np.array([[0.9, 25.0], [0.1, 3.0], [-0.9, -4.0], [0.2, 5.0], [0.3, 6.0], [0.0, 1.0]], np.float32)
    nrm = rng.standard_normal(act.shape).astype(np.float32)
    ev = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    rs = np.array([0, 0, 1, 1, 0, 0], np.uint8)
    x0 = rng.standard_normal(act.shape)
    x = x0.copy() if kind else None
    out, _ = H.host_explore_rows(act, nrm, kind, x, 0.2, low, high, reset=rs, eval_mask=ev)
    # eval rows: the action as it is, out of the box too
    assert np.array_equal(bits(out[ev == 1]), bits(act[ev == 1]))
    # the other rows: the same call without masks, from the state the reset leaves
    xs = None
    if kind:
        xs = x0.copy()
        xs[rs == 1] = 0.0
    ref, _ = H.host_explore_rows(act, nrm, kind, xs, 0.2, low, high)
    assert np.array_equal(bits(out[ev == 0]), bits(ref[ev == 0]))
    assert np.all(out[ev == 0] >= low) and np.all(out[ev == 0] <= high)
    if kind:
        assert np.array_equal(bits(x[0]), bits(x0[0])) and np.array_equal(bits(x[4]), bits(x0[4]))  # eval: untouched
        assert np.all(x[2] == 0.0)  # eval and reset: zeroed, no step
        assert np.array_equal(bits(x[[1, 3, 5]]), bits(xs[[1, 3, 5]]))
        # a reset row starts from 0: x' = 0 + (theta * (mu - 0) * dt + (sigma * sqrt(dt)) * n)
        assert np.array_equal(x[3], 0.0 + (0.15 * (0.0 - 0.0) * 1.0 + (0.2 * np.sqrt(1.0)) * nrm[3].astype(np.float64)))
        assert np.all(x[1] != x0[1])


def test_nan_action_stays_nan_ou(H):
    low, high = np.array([-1.0, -1.0], np.float32), np.array([1.0, 1.0], np.float32)
    act = np.array([[np.nan, 0.5]], np.float32)
    x = np.zeros((1, 2))
    out, _ = H.host_explore_rows(act, np.ones((1, 2), np.float32), 1, x, 0.2, low, high)
    assert np.isnan(out[0, 0]) and out[0, 1] == np.float32(0.5 + 0.2)


# ---- f110_ddpg_actor_explore_env refuses bad arguments before any device call ------------------------
def _explore_env(F, **over):
    """Called with host memory standing in for the device buffers: every case below must be refused
    by the validation, which runs before the first device call (so nothing is ever dereferenced)."""
    B, K, nout = 4, 8, 2
    f = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    st = np.zeros((2, 2), np.float64)
    a = dict(h=f(B, K), W=f(nout, K), b=f(nout), scale=f(nout), shift=f(nout), B=B, K=K, nout=nout, state_in=st[0],
             state_out=st[1], decay=0.999, sigma_min=0.05, low=f(nout), high=f(nout), seed=1, out=f(B, nout),
             out_stride=nout, kind=1, ou_x=np.zeros((B, nout)), theta=0.15, mu=0.0, dt=1.0, reset=None, eval_mask=None,
             normals_ext=None)
    a.update(over)
    P = lambda v: ctypes.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v  # noqa: E731
    L = F.load()
    rc = L.f110_ddpg_actor_explore_env(*[P(a[k]) for k in (
        "h", "W", "b", "scale", "shift", "B", "K", "nout", "state_in", "state_out", "decay", "sigma_min", "low", "high",
        "seed", "out", "out_stride", "kind", "ou_x", "theta", "mu", "dt", "reset", "eval_mask", "normals_ext")], None)
    return rc, (L.f110_last_error() or b"").decode()


_ST = np.zeros(2, np.float64)


@pytest.mark.parametrize("over", [
    dict(kind=2), dict(kind=-1), dict(ou_x=None), dict(dt=-0.5), dict(dt=float("nan")), dict(dt=float("inf")),
    dict(theta=float("nan")), dict(theta=float("inf")), dict(mu=float("nan")), dict(mu=-float("inf")),
    dict(state_in=_ST, state_out=_ST), dict(K=256), dict(nout=5), dict(B=0), dict(out_stride=1),
    dict(kind=0, ou_x=None, dt=-1.0),
], ids=lambda o: ",".join(f"{k}={v if not isinstance(v, np.ndarray) else 'same'}" for k, v in o.items()))
def test_explore_env_refuses_bad_arguments(F, over):
    rc, msg = _explore_env(F, **over)
    assert rc == -1 and "f110_ddpg_actor_explore_env" in msg


def test_host_hook_refuses_bad_arguments(H, F):
    low, high = np.zeros(2, np.float32), np.ones(2, np.float32)
    act = np.zeros((3, 2), np.float32)
    for kw in (dict(kind=2, ou_x=np.zeros((3, 2))), dict(kind=1, ou_x=None), dict(kind=1, ou_x=np.zeros((3, 2)), dt=-1.0),
               dict(kind=1, ou_x=np.zeros((3, 2)), theta=float("nan"))):
        kind, ou_x = kw.pop("kind"), kw.pop("ou_x")
        with pytest.raises(F.F110Error):
            H.host_explore_rows(act, act, kind, ou_x, 0.2, low, high, **kw)


# ---- the learner's torch fallback (no explicit path on the CPU) follows the same semantics -----------
@pytest.mark.parametrize("noise_type", ["gaussian", "ou"])
def test_learner_fallback_rows(H, noise_type):
    torch = pytest.importorskip("torch")
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    kw = dict(obs_dim=12, act_dim=2, action_low=[-0.4189, 0.0], action_high=[0.4189, 20.0], seed=5, device="cpu",
              replay=None, noise_sigma_start=0.2, noise_sigma_min=0.05, noise_decay=0.9, max_add=6)
    ln = DDPGLearner(noise_type=noise_type, ou_dt=0.25, **kw)
    assert ln.explicit is None
    S = torch.randn(6, 12, generator=torch.Generator().manual_seed(1)) * 3
    base = ln.choose_action(S, training=False).clone()
    ev = np.array([0, 1, 0, 0, 1, 0], np.uint8)
    rs = np.array([0, 0, 0, 1, 1, 0], np.uint8)
    kind = 1 if noise_type == "ou" else 0
    xh = np.zeros((6, 2)) if kind else None
    gen = torch.Generator().manual_seed(5)  # the learner's own generator, replayed
    sigma = 0.2
    for call in range(3):
        reset = rs if call == 2 else None
        a = ln.choose_action(S, training=True, eval_mask=torch.from_numpy(ev), reset=reset)
        n = torch.randn(6, 2, generator=gen).numpy()
        ref, (sigma, _) = H.host_explore_rows(base.numpy(), n, kind, xh, sigma, ln.action_low, ln.action_high,
                                              theta=0.15, mu=0.0, dt=0.25, reset=reset, eval_mask=ev, decay=0.9,
                                              sigma_min=0.05)
        assert np.array_equal(bits(a.numpy()), bits(ref)), call
        assert ln.sigma == sigma
        if kind:
            assert np.array_equal(bits(ln.ou_x.numpy()), bits(xh)), call
    assert np.array_equal(bits(a.numpy()[ev == 1]), bits(base.numpy()[ev == 1]))
    # without masks the Gaussian fallback is the path it was
    if not kind:
        lb = DDPGLearner(**kw)
        a = lb.choose_action(S, training=True)
        n = torch.randn(6, 2, generator=torch.Generator().manual_seed(5)) * 0.2
        assert torch.equal(a, torch.clamp(base + n, lb._low, lb._high)) and lb.ou_x is None


def test_best_checkpoint_loads_with_the_safe_loader(tmp_path):
    """save_model writes what load_model's weights_only loader accepts (train.py's best.pt)."""
    torch = pytest.importorskip("torch")
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    kw = dict(obs_dim=12, act_dim=2, action_low=[-0.4189, 0.0], action_high=[0.4189, 20.0], device="cpu", replay=None,
              path=str(tmp_path))
    a, b = DDPGLearner(seed=1, **kw), DDPGLearner(seed=2, **kw)
    a.save_model("best.pt")
    assert b.load_model("best.pt")
    for p, q in zip(a.actor.parameters(), b.actor.parameters()):
        assert torch.equal(p, q)
