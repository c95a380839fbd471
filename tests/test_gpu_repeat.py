"""Action repeat on the device: f110_repeat_hold / f110_repeat_push against the host hooks (which
test_repeat_host.py checks against a model of the rule) through a NumPy ring, repeat = 1 against
add_env, strided inputs, reset, validation, the learner's TD target on the stored effective done for
blocks of 1..64 steps, and VectorTrainer(action_repeat=3) eager against its step graphs.

Shapes (N, obs_dim, K, capacity): obs_dim 6 takes the scalar copy path and 8 / 1088 the float4 one;
N = 70 and 130 are more than one wave of the per-env update kernel; every ring but the 4096-row
one wraps within the 40 pushes."""
import ctypes
import math
import os

import numpy as np
import pytest

from repeat_model import Ring, same_bits, scenario

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

A = 2
SHAPES = [(5, 6, 3, 64), (70, 8, 2, 149), (130, 1088, 4, 4096), (64, 1088, 1, 333)]
KEYS = ("rew", "nxt", "term", "trunc", "reset")


def _buffer(cap, D, max_add=1, seed=5):
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(cap, batch_size=4, obs_dim=D, act_dim=A, device=0, max_add=max_add, seed=seed)


def _rep(N, K, D, gamma=0.99):
    from f110_gymnasium_ros2_jazzy_amd.replay import ActionRepeat
    return ActionRepeat(N, K, gamma, obs_dim=D, act_dim=A, device=0)


def _header(rb):
    ln, nx = ctypes.c_int64(), ctypes.c_int64()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert rb.L.f110_replay_length(rb.handle, ctypes.byref(ln), ctypes.byref(nx), s) == 0
    return ln.value, nx.value


def _dev(sc):
    return {k: torch.from_numpy(v).cuda() for k, v in sc.items()}


def _push_args(d, t):
    return tuple(d[k][t] for k in KEYS)


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


@pytest.mark.parametrize("N,D,K,cap", SHAPES)
def test_device_equals_host_hooks(gpu, N, D, K, cap):
    """After each of 40 holds the action buffer and the decision mask, and after each of 40 pushes
    the ring's six arrays, its header and phase(), equal the host hooks' (a NumPy ring filled from
    their rows), bit for bit; half-way a few priorities change, so the later rows take a max
    priority other than 1.0."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_push, host_repeat_state
    T = 40
    sc = scenario(T, N, D, A, seed=100 * N + K + 4)
    d = _dev(sc)
    rb, rp = _buffer(cap, D), _rep(N, K, D)
    st, ring = host_repeat_state(N, D, A), Ring(cap, D, A)
    try:
        assert rp.phase().tolist() == [0] * N
        total = frac = held = 0
        for t in range(T):
            act = d["act"][t].clone()
            assert rp.hold(d["obs"][t], act) is act
            want_a, want_d = host_repeat_hold(st, sc["obs"][t], sc["act"][t])
            assert same_bits(act.cpu().numpy(), want_a), f"hold {t}"
            assert np.array_equal(rp.decision.cpu().numpy(), want_d), f"hold {t}"
            held += int((want_d == 0).sum())
            rp.push(rb, *_push_args(d, t))
            rows = host_repeat_push(st, K, 0.99, *[sc[k][t] for k in KEYS], capacity=cap)
            ring.add(*rows)
            total += len(rows[2])
            frac += int(((rows[4] > 0) & (rows[4] < 1)).sum())
            _ring_equal(rb, ring, f"push {t}")
            assert np.array_equal(rp.phase().cpu().numpy(), st["k"]), t
            if t == T // 2:
                idx = np.array([0, ring.length // 2, ring.length - 1], np.int64)
                val = np.array([2.5, 0.75, 1.25], np.float32)
                rb.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda())
                ring.a["priority"][idx] = val
        assert sc["term"].sum() and sc["trunc"].sum()
        assert (total > cap and ring.length == cap) == (cap != 4096)  # wrapped
        assert float(ring.a["priority"].max()) == 2.5 and (ring.a["priority"] == 2.5).sum() > 1
        assert (frac > 0) == (K > 1) and (held > 0) == (K > 1)
        w = {k: v.cpu().numpy() for k, v in rp.arrays().items()}
        assert same_bits(w["ret"], st["ret"])  # the returns and the latched rows, finished blocks' included
        assert same_bits(w["obs"], st["obs"]) and same_bits(w["act"], st["act"])
    finally:
        rp.close()
        rb.close()


def test_k1_is_add_env(gpu):
    """repeat = 1 stores what add_env stores and holds nothing: 30 steps at N = 70 into two rings
    of 257 rows."""
    N, D, cap = 70, 12, 257
    d = _dev(scenario(30, N, D, A, seed=7))
    ra, rb_ = _buffer(cap, D, max_add=N), _buffer(cap, D, max_add=N)
    rp = _rep(N, 1, D)
    try:
        for t in range(30):
            s, a = d["obs"][t], d["act"][t]
            r, s2, te, tr, rs = _push_args(d, t)
            ra.add_env(s, a, r, s2, te, rs)
            act = a.clone()
            rp.hold(s, act)
            assert torch.equal(act.view(torch.int32), a.view(torch.int32)) and bool((rp.decision == 1).all())
            rp.push(rb_, r, s2, te, tr, rs)
            if t % 10 == 9:
                ln, _ = _buffers_equal(ra, rb_, f"step {t}")
        assert ln == cap
        assert rp.phase().tolist() == [0] * N
        dn = rb_.arrays(("dones",))["dones"]
        assert bool(((dn == 0) | (dn == 1)).all()) and bool((dn == 1).any())
    finally:
        rp.close()
        ra.close()
        rb_.close()


def test_strided_inputs(gpu):
    """obs as a [N, 1088] view of rows at stride 1152 and act as the [:, 0] view of [N, 2, 2] --
    what F110VectorEnv hands out --, held in place, store what the contiguous tensors store; the
    other agent's rows of the [N, 2, 2] buffer keep their NaN fill."""
    N, D, K, cap = 70, 1088, 3, 512
    T = 10
    d = _dev(scenario(T, N, D, A, seed=9))
    ra, rb_ = _buffer(cap, D), _buffer(cap, D)
    ca, cb = _rep(N, K, D), _rep(N, K, D)
    try:
        held = 0
        for t in range(T):
            s, a = d["obs"][t], d["act"][t]
            r, s2, te, tr, rs = _push_args(d, t)
            wide = torch.full((N, 1152), float("nan"), device="cuda")
            wide2 = torch.full((N, 1152), float("nan"), device="cuda")
            both = torch.full((N, 2, 2), float("nan"), device="cuda")
            wide[:, :D], wide2[:, :D], both[:, 0] = s, s2, a
            assert wide[:, :D].stride(0) == 1152 and both[:, 0].stride(0) == 4
            plain = a.clone()
            ca.hold(s, plain)
            view = both[:, 0]
            assert cb.hold(wide[:, :D], view) is view
            assert torch.equal(both[:, 0].view(torch.int32), plain.view(torch.int32)), t
            assert bool(torch.isnan(both[:, 1]).all()), t
            assert torch.equal(ca.decision, cb.decision)
            held += int((cb.decision == 0).sum())
            ca.push(ra, r, s2, te, tr, rs)
            cb.push(rb_, r, wide2[:, :D], te, tr, rs)
        ln, _ = _buffers_equal(ra, rb_, "strided")
        assert ln > N and held > 0 and torch.equal(ca.phase(), cb.phase())
        assert not bool(torch.isnan(rb_.arrays(("states",))["states"][:ln]).any())
        assert not bool(torch.isnan(rb_.arrays(("next_states",))["next_states"][:ln]).any())
    finally:
        for x in (ca, cb, ra, rb_):
            x.close()


def test_reset_mask(gpu):
    """reset(env_mask) zeroes the masked phases only and stores nothing; the next holds and pushes
    match the host hooks run on a state reset the same way; reset() zeroes all."""
    from f110_gymnasium_ros2_jazzy_amd.replay import host_repeat_hold, host_repeat_push, host_repeat_state
    N, D, K, cap = 70, 8, 4, 512
    T = 12
    sc = scenario(T, N, D, A, seed=13, isolated=())
    sc["term"][:2] = sc["trunc"][:2] = sc["reset"][:3] = 0  # two quiet pushes: every phase is 2
    d = _dev(sc)
    rb, rp = _buffer(cap, D), _rep(N, K, D)
    st, ring = host_repeat_state(N, D, A), Ring(cap, D, A)
    try:
        for t in range(T):
            if t == 2:
                assert rp.phase().tolist() == [2] * N and _header(rb) == (0, 0)
                mask = (np.arange(N) % 3 == 1).astype(np.uint8)
                rp.reset(torch.from_numpy(mask).cuda())
                st["k"][mask != 0] = 0
                assert rp.phase().tolist() == [0 if m else 2 for m in mask] and _header(rb) == (0, 0)
            act = d["act"][t].clone()
            rp.hold(d["obs"][t], act)
            want_a, want_d = host_repeat_hold(st, sc["obs"][t], sc["act"][t])
            assert same_bits(act.cpu().numpy(), want_a) and np.array_equal(rp.decision.cpu().numpy(), want_d), t
            rp.push(rb, *_push_args(d, t))
            ring.add(*host_repeat_push(st, K, 0.99, *[sc[k][t] for k in KEYS]))
            _ring_equal(rb, ring, f"push {t}")
            assert np.array_equal(rp.phase().cpu().numpy(), st["k"]), t
        before = _header(rb)
        assert before[0] > 0
        rp.reset()
        assert rp.phase().tolist() == [0] * N and _header(rb) == before
    finally:
        rp.close()
        rb.close()


def test_validation(gpu):
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.replay import ActionRepeat
    for bad in (dict(repeat=0), dict(repeat=65), dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma=-0.1),
                dict(n_envs=0)):
        kw = dict(n_envs=70, repeat=2, gamma=0.99)
        kw.update(bad)
        with pytest.raises(_lib.F110Error, match="f110_repeat_create"):
            ActionRepeat(kw["n_envs"], kw["repeat"], kw["gamma"], obs_dim=8, act_dim=A, device=0)
    d = _dev(scenario(1, 70, 8, A, seed=1))
    rp = _rep(70, 2, 8)
    small, other = _buffer(69, 8), _buffer(149, 12)
    try:
        s, a = d["obs"][0], d["act"][0].clone()
        r, s2, te, tr, rs = _push_args(d, 0)
        with pytest.raises(ValueError):
            rp.hold(s[:69], a[:69])
        with pytest.raises(TypeError):
            rp.hold(s, a.double())
        with pytest.raises(ValueError):
            rp.hold(s, torch.zeros(70, 2, 2, device="cuda")[:, :, 0])  # inner stride 2: would need a copy
        rp.hold(s, a)
        with pytest.raises(_lib.F110Error, match="capacity"):  # 70 > 69
            rp.push(small, r, s2, te, tr, rs)
        with pytest.raises(_lib.F110Error, match="obs_dim"):
            rp.push(other, r, s2, te, tr, rs)  # a ring of 12-float rows
        with pytest.raises(ValueError):
            rp.push(small, r[:69], s2[:69], te[:69], tr[:69], rs[:69])
        with pytest.raises(TypeError):
            rp.push(small, r.float(), s2, te, tr, rs)
        assert _header(small) == (0, 0) and rp.phase().tolist() == [0] * 70
    finally:
        rp.close()
        small.close()
        other.close()


@pytest.mark.parametrize("gamma", [0.9, 0.99, 0.999])
def test_learner_sees_gamma_k(gpu, gamma):
    """One stored row for each k in 1..64 (repeat = 64, 64 envs; env e ends at its (e + 1)-th push,
    truncated for even e and terminated for odd e): f110_ddpg_td_target on the stored reward and
    effective done against r + gamma^k (1 - done) q in f64, within 2^-23 |q| + 2^-22 (|r| + |q|),
    the bound test_gpu_nstep.py::test_learner_sees_gamma_k derives: the first term for the encoding
    (gamma * (1 - d_eff) is four float32 roundings of values at most 1, each at most 2^-25, away
    from gamma^k -- whatever k is), the second for the kernel's own float32 multiply and add."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import td_target
    N, D, K, H = 64, 4, 64, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    rb, rp = _buffer(64, D), _rep(N, K, D, gamma)
    try:
        env = torch.arange(N, device="cuda")
        for t in range(N):
            ends = env == t
            te = (ends & (env % 2 == 1)).to(torch.uint8)
            tr = (ends & (env % 2 == 0)).to(torch.uint8)
            rs = (env < t).to(torch.uint8)  # an env that has ended stores nothing more
            rp.hold(torch.randn(N, D, device="cuda", generator=g), torch.randn(N, A, device="cuda", generator=g))
            rp.push(rb, torch.randn(N, device="cuda", generator=g, dtype=torch.float64),
                    torch.randn(N, D, device="cuda", generator=g), te, tr, rs)
        assert _header(rb) == (64, 0)
        arr = rb.arrays(("rewards", "dones"))
        r, dn = arr["rewards"], arr["dones"]  # row t: env t, a block of t + 1 steps
        k = np.arange(1, N + 1)
        done = (np.arange(N) % 2 == 1).astype(np.float64)
        assert dn[1::2].tolist() == [1.0] * 32 and dn[0].item() == 0.0 and bool((dn[2::2] > 0).all())
        assert bool((dn[2::2] < 1).all())
        q = torch.randn(N, device="cuda", generator=g) * 10.0
        h = torch.zeros(N, H, device="cuda")
        h[:, 0] = q
        W = torch.zeros(1, H, device="cuda")
        W[0, 0] = 1.0
        y = td_target(h, W, torch.zeros(1, device="cuda"), r, dn, gamma).reshape(-1).double().cpu().numpy()
        r64, q64 = r.double().cpu().numpy(), q.double().cpu().numpy()
        ref = r64 + np.array([math.pow(gamma, int(i)) for i in k]) * (1.0 - done) * q64
        err = np.abs(y - ref)
        bound = 2.0 ** -23 * np.abs(q64) + 2.0 ** -22 * (np.abs(r64) + np.abs(q64))
        print("gamma", gamma, "max err / bound", float((err / bound).max()))
        assert (err <= bound).all()
        assert np.abs(ref - r64)[0::2].min() > 0  # the bootstrap term is there
    finally:
        rp.close()
        rb.close()


@pytest.fixture(scope="module")
def trainer_runs(gpu):
    """VectorTrainer(action_repeat=3) with a 7-step time limit, 24 steps eager and 24 through the
    step graphs; per run the final state and, per step, the env's action rows, the decision mask
    and the step's was_reset / truncated counts."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    old = os.environ.get("F110_STEP_GRAPH")
    runs = []
    try:
        for flag in ("0", "1"):
            os.environ["F110_STEP_GRAPH"] = flag
            tr = VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=3, action_repeat=3, max_episode_steps=7,
                               seed=11)
            try:
                ag = tr.agent
                assert ag.action_repeat == 3 and ag.repeat.n_envs == 64 and ag.gamma == 0.99 and ag.nstep is None
                trunc = pushed = 0
                acts, decs = [], []
                for _ in range(24):
                    tr.step()
                    trunc += int((tr.env.truncated != 0).sum())
                    pushed += int((tr.env.sim.out.was_reset == 0).sum())
                    acts.append(tr.env.agent_actions().clone())
                    decs.append(ag.repeat.decision.clone())
                graphed = None if ag.explicit is None else ((0, True) in tr._sg and (1, True) in tr._sg)
                torch.cuda.synchronize()
                n = len(ag.memory)
                runs.append(dict(ring={k: v[:n].clone() for k, v in ag.memory.arrays().items()},
                                 header=_header(ag.memory), phase=ag.repeat.phase().clone(),
                                 actor=ag._flat["actor"].detach().clone(), trunc=trunc, pushed=pushed, acts=acts,
                                 decs=decs, graphed=graphed, flag=flag))
            finally:
                tr.agent.repeat.close()
                tr.close()
    finally:
        if old is None:
            os.environ.pop("F110_STEP_GRAPH", None)
        else:
            os.environ["F110_STEP_GRAPH"] = old
    return runs


def test_trainer_graphs_match_eager(trainer_runs):
    """The ring, its header, the phases and the actor's weights are identical across the two runs;
    truncations occurred, rows with a fractional done are stored, and fewer rows than steps."""
    a, b = trainer_runs
    for run in trainer_runs:
        assert run["trunc"] > 0
        if run["graphed"] is not None:
            assert run["graphed"] == (run["flag"] == "1")
        assert 0 < run["header"][0] < run["pushed"]
    assert a["header"] == b["header"] and a["pushed"] == b["pushed"]
    for k in a["ring"]:
        assert torch.equal(a["ring"][k].view(torch.int32), b["ring"][k].view(torch.int32)), k
    assert torch.equal(a["phase"], b["phase"])
    assert torch.equal(a["actor"].view(torch.int32), b["actor"].view(torch.int32))
    dn = a["ring"]["dones"]
    assert bool(((dn > 0) & (dn < 1)).any())
    assert set(np.unique(dn.cpu().numpy()).tolist()) <= {0.0, 1.0, float(np.float32(1 - 0.99)),
                                                         float(np.float32(1 - 0.99 * 0.99))}


def test_trainer_holds_actions(trainer_runs):
    """Rows with decision == 0 carry the previous step's action bit for bit; such rows occur, and no
    env shows more than K - 1 = 2 of them in a row."""
    for run in trainer_runs:
        streak = torch.zeros(64, dtype=torch.int64, device="cuda")
        held = 0
        for t, (act, dec) in enumerate(zip(run["acts"], run["decs"])):
            hold = dec == 0
            if t == 0:
                assert not bool(hold.any())  # a fresh handle: every env decides
            else:
                prev = run["acts"][t - 1]
                assert torch.equal(act[hold].view(torch.int32), prev[hold].view(torch.int32)), t
            held += int(hold.sum())
            streak = torch.where(hold, streak + 1, torch.zeros_like(streak))
            assert int(streak.max()) <= 2, t
        assert held > 0
    for x, y in zip(trainer_runs[0]["decs"], trainer_runs[1]["decs"]):
        assert torch.equal(x, y)


def test_lifecycle(gpu):
    """create, one hold + push, destroy, create again: the second round gives equal results."""
    N, D, cap = 70, 8, 128
    d = _dev(scenario(1, N, D, A, seed=21))
    out = []
    for _ in range(2):
        rb, rp = _buffer(cap, D), _rep(N, 1, D)
        try:
            act = d["act"][0].clone()
            rp.hold(d["obs"][0], act)
            rp.push(rb, *_push_args(d, 0))
            hdr = _header(rb)
            out.append((hdr, act.clone(), rp.decision.clone(), rp.phase().clone(),
                        {k: v[:hdr[0]].clone() for k, v in rb.arrays().items()}))
        finally:
            rp.close()
            rb.close()
        assert rp.handle is None
        rp.close()  # a second close is a no-op
    (h0, a0, d0, p0, r0), (h1, a1, d1, p1, r1) = out
    assert h0 == h1 and h0[0] == int((d["reset"][0] == 0).sum()) > 0
    assert torch.equal(a0, a1) and torch.equal(d0, d1) and torch.equal(p0, p1)
    for k in r0:
        assert torch.equal(r0[k].view(torch.int32), r1[k].view(torch.int32)), k
