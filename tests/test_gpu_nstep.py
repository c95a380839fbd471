"""N-step returns on the device: f110_nstep_push against the host hook f110_host_nstep (which
test_nstep_host.py checks against a NumPy model of the rule) through a NumPy ring, n_step = 1
against add_env, strided inputs, reset, the learner's TD target on the stored effective done, and
VectorTrainer(n_step=...) eager against its step graphs.

Shapes (N, obs_dim, n, capacity): obs_dim 6 takes the scalar copy path and 8 / 1088 the float4 one;
N = 70 and 130 are more than one wave, 130 at n = 5 gives 650 (env, row) blocks; every ring wraps
several times in 40 pushes.  The issue's second shape, (70, 8, 2, 97), contradicts its own rule
n_envs * n_step <= capacity (140 > 97): the capacity here is 149, also odd and wrapped about 18
times, and test_push_validation checks that the 97-row ring is refused."""
import ctypes
import math

import numpy as np
import pytest

from nstep_model import Ring, live_entries, same_bits, scenario

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

A = 2
SHAPES = [(5, 6, 3, 64), (70, 8, 2, 149), (130, 1088, 5, 4096), (64, 1088, 1, 333)]


def _buffer(cap, D, max_add=1, seed=5):
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(cap, batch_size=4, obs_dim=D, act_dim=A, device=0, max_add=max_add, seed=seed)


def _acc(N, n, D, gamma=0.99):
    from f110_gymnasium_ros2_jazzy_amd.replay import NStepAccumulator
    return NStepAccumulator(N, n, gamma, obs_dim=D, act_dim=A, device=0)


def _header(rb):
    ln, nx = ctypes.c_int64(), ctypes.c_int64()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert rb.L.f110_replay_length(rb.handle, ctypes.byref(ln), ctypes.byref(nx), s) == 0
    return ln.value, nx.value


def _dev(sc):
    return {k: torch.from_numpy(v).cuda() for k, v in sc.items()}


def _step(d, t):
    return d["obs"][t], d["act"][t], d["rew"][t], d["nxt"][t], d["term"][t], d["trunc"][t], d["reset"][t]


def _ring_equal(rb, ring, what):
    """The stored rows (the first `length` slots: the rest was never written) and the header."""
    assert _header(rb) == (ring.length, ring.next), what
    arr = rb.arrays()
    for name in Ring.NAMES:
        got = arr[name][:ring.length].cpu().numpy()
        assert same_bits(got, ring.a[name][:ring.length]), f"{name}, {what}"


def _buffers_equal(ra, rb_, what):
    ha, hb = _header(ra), _header(rb_)
    assert ha == hb, what
    aa, ab = ra.arrays(), rb_.arrays()
    for name in Ring.NAMES:
        assert torch.equal(aa[name][:ha[0]].view(torch.int32), ab[name][:ha[0]].view(torch.int32)), f"{name}, {what}"
    return ha


@pytest.mark.parametrize("N,D,n,cap", SHAPES)
def test_device_equals_host_hook(gpu, N, D, n, cap):
    """After every one of 40 pushes the ring's six arrays and header equal a NumPy ring filled from
    the host hook's rows, and pending() its window lengths, bit for bit; half-way a few priorities
    change, so the later rows take a max priority other than 1.0."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    T = 40
    sc = scenario(T, N, D, A, seed=100 * N + n)
    d = _dev(sc)
    rb, acc = _buffer(cap, D), _acc(N, n, D)
    st, ring = host_nstep_state(N, n, D, A), Ring(cap, D, A)
    try:
        assert acc.pending().tolist() == [0] * N
        frac = 0
        for t in range(T):
            acc.push(rb, *_step(d, t))
            rows = host_nstep(st, 0.99, *[sc[k][t] for k in ("obs", "act", "rew", "nxt", "term", "trunc", "reset")],
                              capacity=cap)
            ring.add(*rows)
            frac += int(((rows[4] > 0) & (rows[4] < 1)).sum())
            _ring_equal(rb, ring, f"push {t}")
            assert np.array_equal(acc.pending().cpu().numpy(), st["len"]), t
            if t == T // 2:
                idx = np.array([0, ring.length // 2, ring.length - 1], np.int64)
                val = np.array([2.5, 0.75, 1.25], np.float32)
                rb.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda())
                ring.a["priority"][idx] = val
        assert ring.length == cap and sc["term"].sum() and sc["trunc"].sum()  # wrapped
        assert float(ring.a["priority"].max()) == 2.5 and (ring.a["priority"] == 2.5).sum() > 1
        assert (frac > 0) == (n > 1)
        w = {k: v.cpu().numpy() for k, v in acc.arrays().items()}
        for a_, b_ in zip(live_entries(w), live_entries(st)):
            assert same_bits(a_, b_)
        for e in range(N):  # the pending entries' rows
            for i in range(int(st["len"][e])):
                s = (int(st["head"][e]) + i) % n
                assert int(w["head"][e]) == int(st["head"][e])
                assert same_bits(w["obs"][e, s], st["obs"][e, s]) and same_bits(w["act"][e, s], st["act"][e, s])
    finally:
        acc.close()
        rb.close()


def test_n1_is_add_env(gpu):
    """n_step = 1 stores what add_env stores: 30 steps at N = 70 into two rings of 257 rows."""
    N, D, cap = 70, 12, 257
    d = _dev(scenario(30, N, D, A, seed=7))
    ra, rb_ = _buffer(cap, D, max_add=N), _buffer(cap, D, max_add=N)
    acc = _acc(N, 1, D)
    try:
        for t in range(30):
            s, a, r, s2, te, tr, rs = _step(d, t)
            ra.add_env(s, a, r, s2, te, rs)
            acc.push(rb_, s, a, r, s2, te, tr, rs)
            if t % 10 == 9:
                ln, _ = _buffers_equal(ra, rb_, f"step {t}")
        assert ln == cap
        assert acc.pending().tolist() == [0] * N
        dn = rb_.arrays(("dones",))["dones"]
        assert bool(((dn == 0) | (dn == 1)).all()) and bool((dn == 1).any())
    finally:
        acc.close()
        ra.close()
        rb_.close()


def test_strided_inputs(gpu):
    """obs as a [N, 1088] view of rows at stride 1152 and act as the [:, 0, :] view of [N, 2, 2] --
    what F110VectorEnv hands out -- store what the contiguous tensors store."""
    N, D, n, cap = 70, 1088, 3, 512
    T = 10
    d = _dev(scenario(T, N, D, A, seed=9))
    ra, rb_ = _buffer(cap, D), _buffer(cap, D)
    ca, cb = _acc(N, n, D), _acc(N, n, D)
    try:
        for t in range(T):
            s, a, r, s2, te, tr, rs = _step(d, t)
            wide = torch.full((N, 1152), float("nan"), device="cuda")
            wide2 = torch.full((N, 1152), float("nan"), device="cuda")
            both = torch.full((N, 2, 2), float("nan"), device="cuda")
            wide[:, :D], wide2[:, :D], both[:, 0] = s, s2, a
            assert wide[:, :D].stride(0) == 1152 and both[:, 0].stride(0) == 4
            ca.push(ra, s, a, r, s2, te, tr, rs)
            cb.push(rb_, wide[:, :D], both[:, 0], r, wide2[:, :D], te, tr, rs)
        ln, _ = _buffers_equal(ra, rb_, "strided")
        assert ln > N and torch.equal(ca.pending(), cb.pending())
        assert not bool(torch.isnan(rb_.arrays(("states",))["states"][:ln]).any())
    finally:
        for x in (ca, cb, ra, rb_):
            x.close()


def test_reset_mask(gpu):
    """reset(env_mask) empties the masked windows only and stores nothing; the next pushes match the
    host hook run on windows emptied the same way; reset() empties all."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_nstep, host_nstep_state
    N, D, n, cap = 70, 8, 4, 512
    T = 12
    sc = scenario(T, N, D, A, seed=13, isolated=())
    sc["term"][:3] = sc["trunc"][:3] = sc["reset"][:4] = 0  # three quiet pushes: every window holds 3 entries
    d = _dev(sc)
    rb, acc = _buffer(cap, D), _acc(N, n, D)
    st, ring = host_nstep_state(N, n, D, A), Ring(cap, D, A)
    try:
        for t in range(T):
            if t == 3:
                assert acc.pending().tolist() == [3] * N and _header(rb) == (0, 0)
                mask = (np.arange(N) % 3 == 1).astype(np.uint8)
                acc.reset(torch.from_numpy(mask).cuda())
                st["len"][mask != 0] = 0
                st["head"][mask != 0] = 0
                assert acc.pending().tolist() == [0 if m else 3 for m in mask] and _header(rb) == (0, 0)
            acc.push(rb, *_step(d, t))
            ring.add(*host_nstep(st, 0.99, *[sc[k][t] for k in ("obs", "act", "rew", "nxt", "term", "trunc", "reset")]))
            _ring_equal(rb, ring, f"push {t}")
            assert np.array_equal(acc.pending().cpu().numpy(), st["len"]), t
        before = _header(rb)
        acc.reset()
        assert acc.pending().tolist() == [0] * N and _header(rb) == before
    finally:
        acc.close()
        rb.close()


def test_push_validation(gpu):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.replay import NStepAccumulator
    for bad in (dict(n_step=0), dict(n_step=17), dict(gamma=1.5), dict(gamma=float("nan")), dict(n_envs=0)):
        kw = dict(n_envs=70, n_step=2, gamma=0.99)
        kw.update(bad)
        with pytest.raises(_lib.F110Error, match="f110_nstep_create"):
            NStepAccumulator(kw["n_envs"], kw["n_step"], kw["gamma"], obs_dim=8, act_dim=A, device=0)
    d = _dev(scenario(1, 70, 8, A, seed=1))
    acc = _acc(70, 2, 8)
    small, other = _buffer(97, 8), _buffer(149, 12)
    try:
        with pytest.raises(_lib.F110Error, match="capacity"):  # 70 * 2 > 97
            acc.push(small, *_step(d, 0))
        with pytest.raises(_lib.F110Error, match="obs_dim"):
            acc.push(other, *_step(d, 0))  # a ring of 12-float rows
        with pytest.raises(ValueError):
            acc.push(small, *[x[:69] for x in _step(d, 0)])
        with pytest.raises(TypeError):
            s, a, r, s2, te, tr, rs = _step(d, 0)
            acc.push(small, s, a, r.float(), s2, te, tr, rs)
        assert _header(small) == (0, 0) and acc.pending().tolist() == [0] * 70
    finally:
        acc.close()
        small.close()
        other.close()


@pytest.mark.parametrize("gamma", [0.9, 0.99, 0.999])
def test_learner_sees_gamma_k(gpu, gamma):
    """Rows with k = 1..16 and done in {0, 1}, stored by the accumulator (env 0 truncates at its
    16th push, env 1 terminates): f110_ddpg_td_target on the stored reward and effective done
    against r + gamma^k (1 - done) q in f64, within 2^-23 |q| + 2^-22 (|r| + |q|): the first term
    for the encoding (gamma * (1 - d_eff) is four float32 roundings of values at most 1, each at
    most 2^-25, away from gamma^k), the second for the kernel's own float32 multiply and add."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import td_target
    N, D, n, K = 2, 4, 16, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    rb, acc = _buffer(64, D), _acc(N, n, D, gamma)
    try:
        zero = torch.zeros(N, dtype=torch.uint8, device="cuda")
        for t in range(16):
            last = t == 15
            te = torch.tensor([0, int(last)], dtype=torch.uint8, device="cuda")
            tr = torch.tensor([int(last), 0], dtype=torch.uint8, device="cuda")
            acc.push(rb, torch.randn(N, D, device="cuda", generator=g), torch.randn(N, A, device="cuda", generator=g),
                     torch.randn(N, device="cuda", generator=g, dtype=torch.float64), torch.randn(N, D, device="cuda", generator=g),
                     te, tr, zero)
        assert _header(rb) == (32, 32)
        arr = rb.arrays(("rewards", "dones"))
        r, dn = arr["rewards"][:32], arr["dones"][:32]
        k = np.concatenate([np.arange(16, 0, -1)] * 2)        # oldest first: 16 rewards .. 1
        done = np.repeat([0.0, 1.0], 16)
        assert dn[16:].tolist() == [1.0] * 16 and dn[15].item() == 0.0 and bool((dn[:15] > 0).all())
        q = torch.randn(32, device="cuda", generator=g) * 10.0
        h = torch.zeros(32, K, device="cuda")
        h[:, 0] = q
        W = torch.zeros(1, K, device="cuda")
        W[0, 0] = 1.0
        y = td_target(h, W, torch.zeros(1, device="cuda"), r, dn, gamma).reshape(-1).double().cpu().numpy()
        r64, q64 = r.double().cpu().numpy(), q.double().cpu().numpy()
        ref = r64 + np.array([math.pow(gamma, int(i)) for i in k]) * (1.0 - done) * q64
        err = np.abs(y - ref)
        bound = 2.0 ** -23 * np.abs(q64) + 2.0 ** -22 * (np.abs(r64) + np.abs(q64))
        print("gamma", gamma, "max err / bound", float((err / bound).max()))
        assert (err <= bound).all()
        assert np.abs(ref - r64)[:16].min() > 0  # the bootstrap term is there
    finally:
        acc.close()
        rb.close()


def _trainer_state(tr):
    ag = tr.agent
    torch.cuda.synchronize()
    n = len(ag.memory)
    ring = {k: v[:n].clone() for k, v in ag.memory.arrays().items()}
    return ring, _header(ag.memory), ag.nstep.pending().clone(), ag._flat["actor"].detach().clone()


def test_trainer_graphs_match_eager(gpu, monkeypatch):
    """VectorTrainer(n_step=3) with a 7-step time limit, 24 steps eager and 24 through the step
    graphs: the ring, its header, the windows' lengths and the actor's weights are identical;
    truncations occurred and rows with a fractional done are stored."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    runs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("F110_STEP_GRAPH", flag)
        tr = VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=3, n_step=3, max_episode_steps=7, seed=11)
        try:
            assert tr.agent.n_step == 3 and tr.agent.nstep.n_envs == 64 and tr.agent.gamma == 0.99
            trunc = 0
            for _ in range(24):
                tr.step()
                trunc += int((tr.env.truncated != 0).sum())
            assert trunc > 0
            if tr.agent.explicit is not None:
                assert ((0, True) in tr._sg and (1, True) in tr._sg) == (flag == "1")
            runs.append(_trainer_state(tr))
        finally:
            tr.agent.nstep.close()
            tr.close()
    (ra, ha, pa, wa), (rb_, hb, pb, wb) = runs
    assert ha == hb and ha[0] > 64 * 15
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb_[k].view(torch.int32)), k
    assert torch.equal(pa, pb) and torch.equal(wa.view(torch.int32), wb.view(torch.int32))
    dn = ra["dones"]
    assert bool(((dn > 0) & (dn < 1)).any()) and bool((dn == 0).any())
    assert set(np.unique(dn.cpu().numpy()).tolist()) <= {0.0, 1.0, float(np.float32(1 - 0.99)),
                                                         float(np.float32(1 - 0.99 * 0.99))}


def test_trainer_default_is_add_env(gpu, monkeypatch):
    """The default n_step = 1 creates no accumulator and stores what add_env stores: the trainer's
    ring against a second ring fed the same transitions (and the same priority updates) directly."""
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    tr = VectorTrainer(16, batch_size=16, memory_size=256, warmup_steps=2)
    ag = tr.agent
    mem = ag.memory
    twin = DeviceReplayBuffer(256, batch_size=16, obs_dim=mem.obs_dim, act_dim=2, device=0, max_add=16)
    calls = []
    add_env, update = mem.add_env, mem.update_priorities

    def add_env_both(*a):
        calls.append(len(a))
        twin.add_env(*a)
        return add_env(*a)

    def update_both(*a, **kw):
        twin.update_priorities(*a, **kw)
        return update(*a, **kw)
    monkeypatch.setattr(mem, "add_env", add_env_both)
    monkeypatch.setattr(mem, "update_priorities", update_both)
    try:
        assert ag.n_step == 1 and ag.nstep is None
        for _ in range(5):  # 2 warm-up steps and the learner's 3 eager updates: every call goes through Python
            tr.step()
        assert calls == [6] * 5 and ag._graphs is None and tr._sg == {}
        torch.cuda.synchronize()
        ln, _ = _buffers_equal(mem, twin, "default trainer")
        assert 40 <= ln <= 80  # 5 x 16 rows less the reset rows
    finally:
        twin.close()
        tr.close()
