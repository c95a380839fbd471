"""f110_ddpg_actor_explore_env on the device: the per-row exploration head (Gaussian or OU noise,
eval rows, reset rows, caller-supplied draws) against the existing entry points, the host hook
f110_host_explore_rows and the reference's OUActionNoise (tests/golden/ou_noise.npz), and
VectorTrainer's noise_type / eval_envs / ou_reset keywords that run it inside the step graphs.

Shapes: B in {1, 5, 67} (8 rows per block: 67 leaves a partial block), K in {128, 18} (18 is no
multiple of 4: the scalar load path), nout in {2, 3} (3 leaves an odd pair of draws)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ou_noise.npz")
SHAPES = [(B, K, n) for B in (1, 5, 67) for K in (128, 18) for n in (2, 3)]
LOW = [-0.4189, 0.0, -1.0]
HIGH = [0.4189, 20.0, 1.0]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Case:
    """One head problem: h [B, K], fc3's W [nout, K] and b, the action box.  The pre-activations
    spread over about +-2, so tanh reaches its flat ends and part of the noisy actions clip."""

    def __init__(self, B, K, nout, seed=0, low=None, high=None):
        g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * K + nout + seed)
        self.B, self.K, self.n = B, K, nout
        self.h = torch.randn(B, K, device="cuda", generator=g).relu()
        self.W = torch.randn(nout, K, device="cuda", generator=g) * (2.0 / K ** 0.5)
        self.b = torch.randn(nout, device="cuda", generator=g) * 0.1
        self.low = torch.tensor(LOW[:nout] if low is None else low, device="cuda", dtype=torch.float32)
        self.high = torch.tensor(HIGH[:nout] if high is None else high, device="cuda", dtype=torch.float32)
        self.scale = 0.5 * (self.high - self.low)
        self.shift = 0.5 * (self.high + self.low)

    def head(self):
        """f110_ddpg_actor_head's act."""
        from f110_gymnasium_ros2_jazzy_amd import _lib
        act = torch.empty(self.B, self.n, device="cuda")
        t = torch.empty(self.B, self.n, device="cuda")
        _lib.check(_lib.load().f110_ddpg_actor_head(_p(self.h), _p(self.W), _p(self.b), _p(self.scale), _p(self.shift),
                                                    self.B, self.K, self.n, _p(act), _p(t), _stream()))
        return act

    def explore(self, st_in, st_out, decay, sigma_min, seed, out):
        """The existing entry point, f110_ddpg_actor_explore."""
        from f110_gymnasium_ros2_jazzy_amd import _lib
        _lib.check(_lib.load().f110_ddpg_actor_explore(
            _p(self.h), _p(self.W), _p(self.b), _p(self.scale), _p(self.shift), self.B, self.K, self.n, _p(st_in),
            _p(st_out), decay, sigma_min, _p(self.low), _p(self.high), seed, _p(out), out.stride(0), _stream()))
        return out

    def explore_env(self, st_in, st_out, decay, sigma_min, seed, out, **kw):
        from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import actor_explore_env
        return actor_explore_env(self.h, self.W, self.b, self.scale, self.shift, st_in, st_out, decay, sigma_min,
                                 self.low, self.high, seed, out, **kw)

    def strided_out(self):
        """A NaN-filled [B, 3, nout] buffer and its middle [B, nout] view (row stride 3 * nout)."""
        buf = torch.full((self.B, 3, self.n), float("nan"), device="cuda")
        return buf, buf[:, 1]


def st(sigma, call):
    return torch.tensor([sigma, float(call)], dtype=torch.float64, device="cuda")


def untouched(buf):
    return bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, 2]).all())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def masks(B):
    """Eval rows 0, 3, 6, ...; reset rows 0, 1, 5, 6, 10, ... (every combination of the two occurs
    from B = 5 on; B = 1 is one eval + reset row)."""
    i = torch.arange(B, device="cuda")
    return (i % 3 == 0).to(torch.uint8), (i % 5 < 2).to(torch.uint8)


@pytest.mark.parametrize("B,K,nout", SHAPES)
def test_gaussian_equals_existing_entry(gpu, B, K, nout):
    """Kind 0 without masks or external draws is f110_ddpg_actor_explore bit for bit: actions (into a
    strided out) and the decayed state pair."""
    c = Case(B, K, nout)
    for sigma, call in ((0.2, 0), (0.05, 2 ** 33 + 5)):
        nx_a, nx_b = st(0, 0), st(0, 0)
        buf_a, out_a = c.strided_out()
        buf_b, out_b = c.strided_out()
        c.explore(st(sigma, call), nx_a, 0.9, 0.02, 77, out_a)
        c.explore_env(st(sigma, call), nx_b, 0.9, 0.02, 77, out_b, kind=0)
        assert not bool(torch.isnan(out_a).any())
        assert same_bits(out_a, out_b)
        assert untouched(buf_b)
        assert nx_a.tolist() == nx_b.tolist() == [max(sigma * 0.9, 0.02), float(call + 1)]
    if B * nout >= 10:  # the noise is there
        assert not torch.equal(out_b, c.head())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B,K,nout", SHAPES)
def test_eval_rows(gpu, B, K, nout, kind):
    """Eval rows get f110_ddpg_actor_head's act bit for bit (unclipped: the box here is narrower than
    the actor's range), the other rows what the same call gives without a mask; nothing outside out's
    columns is written; an eval row's OU state stays as it is."""
    c = Case(B, K, nout)
    act = c.head()
    c.low, c.high = c.low * 0.5, c.high * 0.5  # the clip box only: scale / shift keep the actor's range
    ev, _ = masks(B)
    evb = ev.bool()
    g = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(B, nout, device="cuda", generator=g, dtype=torch.float64) if kind else None
    xa, xb = (x0.clone(), x0.clone()) if kind else (None, None)
    buf_a, out_a = c.strided_out()
    buf_b, out_b = c.strided_out()
    nx = st(0, 0)
    c.explore_env(st(0.2, 3), nx, 0.9, 0.02, 9, out_a, kind=kind, ou_x=xa, eval_mask=ev)
    c.explore_env(st(0.2, 3), nx, 0.9, 0.02, 9, out_b, kind=kind, ou_x=xb)
    assert untouched(buf_a) and untouched(buf_b)
    assert same_bits(out_a[evb], act[evb])
    assert bool(((act[evb] < c.low) | (act[evb] > c.high)).any()) or B < 67  # some of them lie outside the box
    assert same_bits(out_a[~evb], out_b[~evb])
    assert bool(((out_b >= c.low) & (out_b <= c.high)).all())
    if kind:
        assert same_bits(xa[evb], x0[evb]) and same_bits(xa[~evb], xb[~evb])
        assert not bool((xb == x0).any())


@pytest.mark.parametrize("name,K", [("A", 128), ("B", 18)])
def test_ou_matches_host_hook_and_reference(gpu, name, K):
    """The golden scenarios call by call, with the golden's draws as normals_ext and its reset rows:
    the OU state equals the host hook's and the reference's bit for bit; the actions, whose act
    comes from the head here, equal the host hook fed f110_ddpg_actor_head's output."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import host_explore_rows
    with np.load(GOLDEN) as z:
        G = {k[2:]: z[k] for k in z.files if k.startswith(name + "_")}
    theta, mu, dt, sigma, sigma_min, decay = G["hyper"].tolist()
    calls, rows, nout = G["act"].shape
    x = torch.zeros(rows, nout, dtype=torch.float64, device="cuda")
    xh = np.zeros((rows, nout), np.float64)
    pair = [st(sigma, 0), st(0, 0)]
    clipped = 0
    for k in range(calls):
        c = Case(rows, K, nout, seed=k, low=G["low"].tolist(), high=G["high"].tolist())
        c.scale, c.shift = c.scale * 1.15, c.shift  # actions past the box, as the golden's
        act = c.head()
        out = torch.empty(rows, nout, device="cuda")
        assert pair[k & 1].tolist() == [G["sigma"][k], float(k)]
        c.explore_env(pair[k & 1], pair[1 - (k & 1)], decay, sigma_min, 1, out, kind=1, ou_x=x, theta=theta, mu=mu,
                      dt=dt, reset=torch.from_numpy(G["reset"][k]).cuda(),
                      normals_ext=torch.from_numpy(G["normals"][k]).cuda())
        ref, _ = host_explore_rows(act.cpu().numpy(), G["normals"][k], 1, xh, float(G["sigma"][k]), G["low"],
                                   G["high"], theta=theta, mu=mu, dt=dt, reset=G["reset"][k])
        xd = x.cpu().numpy()
        assert np.array_equal(xd.view(np.uint64), G["x"][k].view(np.uint64)), f"x vs the reference, call {k}"
        assert np.array_equal(xd.view(np.uint64), xh.view(np.uint64)), f"x vs the host hook, call {k}"
        o = out.cpu().numpy()
        assert np.array_equal(o.view(np.uint32), ref.view(np.uint32)), f"actions, call {k}"
        clipped += int(((o == G["low"]) | (o == G["high"])).sum())
    assert pair[calls & 1].tolist() == [G["sigma"][calls], float(calls)]
    assert clipped > 0


@pytest.mark.parametrize("B,K,nout", SHAPES)
def test_ou_matches_host_hook(gpu, B, K, nout):
    """Every shape, three calls with eval and reset rows and external draws: actions and state equal
    the host hook's bit for bit."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg_heads import host_explore_rows
    c = Case(B, K, nout)
    act = c.head().cpu().numpy()
    ev, rs = masks(B)
    g = torch.Generator(device="cuda").manual_seed(B + K)
    x = torch.randn(B, nout, device="cuda", generator=g, dtype=torch.float64)
    xh = x.cpu().numpy().copy()
    sigma, pair = 0.3, [st(0.3, 0), st(0, 0)]
    for k in range(3):
        nrm = torch.randn(B, nout, device="cuda", generator=g)
        reset = rs if k == 1 else None
        buf, out = c.strided_out()
        c.explore_env(pair[k & 1], pair[1 - (k & 1)], 0.5, 0.1, 3, out, kind=1, ou_x=x, theta=0.15, mu=0.0, dt=0.01,
                      reset=reset, eval_mask=ev, normals_ext=nrm)
        ref, (sigma, _) = host_explore_rows(act, nrm.cpu().numpy(), 1, xh, sigma, c.low.cpu().numpy(),
                                            c.high.cpu().numpy(), theta=0.15, mu=0.0, dt=0.01,
                                            reset=None if reset is None else reset.cpu().numpy(),
                                            eval_mask=ev.cpu().numpy(), decay=0.5, sigma_min=0.1, call=k)
        assert untouched(buf)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), k
        assert np.array_equal(x.cpu().numpy().view(np.uint64), xh.view(np.uint64)), k
        assert pair[1 - (k & 1)].tolist() == [sigma, float(k + 1)]


@pytest.mark.parametrize("B,K,nout", SHAPES)
def test_ou_draws_its_own_normals(gpu, B, K, nout):
    """theta = 0, sigma = 1, dt = 1 from x = 0 with a zero actor and no box: x' is the draw itself, and
    so is kind 0's action -- both kinds draw the same normals for (seed, call, row, output); eval rows
    do not shift the others' draws; another call index draws anew."""
    c = Case(B, K, nout, low=[-1e30] * nout, high=[1e30] * nout)
    c.scale, c.shift = torch.zeros_like(c.scale), torch.zeros_like(c.shift)
    nx = st(0, 0)

    def ou(call, ev=None):
        x = torch.zeros(B, nout, dtype=torch.float64, device="cuda")
        out = torch.empty(B, nout, device="cuda")
        c.explore_env(st(1.0, call), nx, 1.0, 1.0, 21, out, kind=1, ou_x=x, theta=0.0, mu=0.0, dt=1.0, eval_mask=ev)
        return x, out

    n0 = c.explore_env(st(1.0, 4), nx, 1.0, 1.0, 21, torch.empty(B, nout, device="cuda"), kind=0)
    assert nx.tolist() == [1.0, 5.0]
    x4, o4 = ou(4)
    assert torch.equal(x4, n0.double()) and torch.equal(o4, n0)
    assert bool((n0 != 0).all()) and float(n0.abs().max()) < 6.0
    x5, _ = ou(5)
    assert not bool((x5 == x4).any())
    ev, _ = masks(B)
    xe, oe = ou(4, ev)
    assert torch.equal(xe[~ev.bool()], x4[~ev.bool()]) and bool((xe[ev.bool()] == 0).all())
    assert bool((oe[ev.bool()] == 0).all())


def test_learner_choose_action_rows(gpu):
    """DDPGLearner(noise_type="ou").choose_action: eval rows are the training=False rows, reset rows
    start from 0, the host mirror follows the device pair; noise_type="gaussian" without masks keeps
    drawing what f110_ddpg_actor_explore draws."""
    from f110_gymnasium_ros2_jazzy_amd.ddpg import DDPGLearner
    kw = dict(obs_dim=64, act_dim=2, action_low=[-0.4189, 0.0], action_high=[0.4189, 20.0], seed=9, device="cuda:0",
              replay=None, noise_sigma_start=0.2, noise_sigma_min=0.02, noise_decay=0.9, max_add=67)
    ln = DDPGLearner(noise_type="ou", **kw)
    if ln.explicit is None:
        pytest.skip("explicit learner path not supported here")
    assert ln.ou_x.shape == (67, 2) and ln.ou_x.dtype == torch.float64
    g = torch.Generator(device="cuda").manual_seed(2)
    S = torch.randn(67, 64, device="cuda", generator=g)
    base = ln.choose_action(S, training=False).clone()
    ev, rs = masks(67)
    a1 = ln.choose_action(S, training=True, eval_mask=ev).clone()
    x1 = ln.ou_x.clone()
    assert same_bits(a1[ev.bool()], base[ev.bool()]) and not bool((a1[~ev.bool()] == base[~ev.bool()]).all())
    assert bool((x1[ev.bool()] == 0).all()) and bool((x1[~ev.bool()] != 0).all())
    ln.choose_action(S, training=True, eval_mask=ev.bool(), reset=rs)
    torch.cuda.synchronize()
    x2 = ln.ou_x
    only_rs = rs.bool() & ~ev.bool()
    sg = 0.2 * 0.9
    assert bool((x2[only_rs].abs() < 6 * sg).all()) and bool((x2[rs.bool() & ev.bool()] == 0).all())
    assert ln._noise_state[ln._noise_slot].tolist() == [ln.sigma, 2.0] and ln.sigma == 0.2 * 0.9 * 0.9
    with pytest.raises(ValueError):
        ln.choose_action(torch.zeros(68, 64, device="cuda"), training=True)
    with pytest.raises(ValueError):
        DDPGLearner(noise_type="pink", **kw)
    # Gaussian, no masks: the existing launch; with an all-zero eval mask: the new one, same draws
    la, lb = DDPGLearner(**kw), DDPGLearner(**kw)
    ga = la.choose_action(S, training=True)
    gb = lb.choose_action(S, training=True, eval_mask=torch.zeros(67, dtype=torch.uint8, device="cuda"))
    assert same_bits(ga, gb) and la.sigma == lb.sigma and lb.ou_x is None


def _trainer_run(monkeypatch, flag, steps, **kw):
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer
    monkeypatch.setenv("F110_STEP_GRAPH", flag)
    return VectorTrainer(64, batch_size=64, memory_size=4096, warmup_steps=3, noise_type="ou", eval_envs=8, seed=11,
                         **kw)


def test_trainer_eval_rows_and_graphs_match_eager(gpu, monkeypatch):
    """VectorTrainer(noise_type="ou", eval_envs=8): at every step, warm-up included, the eval envs act
    on the actor's noise-free action (choose_action(training=False) on the full batch, taken before
    the step); the training rows differ from it after the warm-up; and 14 steps leave the weights,
    the replay ring, the OU state, the noise pair and the losses bit-identical between the step
    graphs and the eager loop."""
    runs = []
    for flag in ("1", "0"):
        tr = _trainer_run(monkeypatch, flag, 14)
        try:
            ag = tr.agent
            if ag.explicit is None:
                pytest.skip("explicit learner path not supported here")
            assert tr.episode_stats and tr.env._episode is None
            for k in range(14):
                want = ag.choose_action(tr.obs, training=False).clone()
                tr.step()
                got = tr.env.agent_actions()
                assert same_bits(got[56:], want[56:]), f"eval rows, step {k}"
                if k >= 3:
                    assert not bool((got[:56] == want[:56]).all(1).any()), f"training rows, step {k}"
            torch.cuda.synchronize()
            assert ((0, True) in tr._sg and (1, True) in tr._sg) == (flag == "1")
            assert bool((ag.ou_x[56:] == 0).all()) and bool((ag.ou_x[:56] != 0).all())
            params = [p.detach().clone() for p in list(ag.actor.parameters()) + list(ag.critic.parameters())]
            n = len(ag.memory)
            ring = {k: v[:n].clone() for k, v in ag.memory.arrays().items()}
            runs.append((params, ring, ag.ou_x.clone(), ag._noise_state[ag._noise_slot].tolist(),
                         (ag.sigma, ag._noise_calls, n, float(tr.last["critic_loss"]), float(tr.last["actor_loss"]))))
        finally:
            tr.close()
    (pa, ra, xa, sa, ha), (pb, rb, xb, sb, hb) = runs
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert same_bits(xa, xb) and sa == sb and ha == hb
    assert sa == [ha[0], float(ha[1])] and ha[1] == 11  # one noise call per step after the warm-up


def test_trainer_eval_statistics_and_ou_reset(gpu, monkeypatch):
    """max_episode_steps=20 over 80 steps with ou_reset=True: episode_report splits the finished
    episodes into the training and the eval rows, whose counts add up to the finishes counted from
    the step flags; and on the step after a row's was_reset its OU state is 0 plus that step's dx
    (the draw recovered through kind 0 with a zero actor, as in test_ou_draws_its_own_normals)."""
    from f110_gymnasium_ros2_jazzy_amd.train import episode_report
    tr = _trainer_run(monkeypatch, "1", 80, max_episode_steps=20, ou_reset=True)
    try:
        ag = tr.agent
        if ag.explicit is None:
            pytest.skip("explicit learner path not supported here")
        c = Case(64, 128, 2, low=[-1e30] * 2, high=[1e30] * 2)
        c.scale, c.shift = torch.zeros_like(c.scale), torch.zeros_like(c.shift)
        fin = np.zeros(64, np.int64)
        checked = 0
        for k in range(80):
            was_prev = tr.env.sim.out.was_reset.clone().bool()
            sigma, call = ag.sigma, ag._noise_calls
            tr.step()
            out = tr.env.sim.out
            was = out.was_reset.bool()
            fin += (((out.terminated != 0) | (tr.env.truncated != 0)) & ~was).cpu().numpy()
            rows = was_prev[:56].nonzero().flatten()
            if k >= 3 and len(rows):
                n = c.explore_env(st(1.0, call), st(0, 0), 1.0, 1.0, ag._noise_key, torch.empty(64, 2, device="cuda"),
                                  kind=0).double()
                want = 0.0 + (ag.ou_theta * (ag.ou_mu - 0.0) * ag.ou_dt + (sigma * 1.0) * n)
                assert same_bits(ag.ou_x[rows], want[rows]), f"step {k}"
                rest = (~was_prev[:56]).nonzero().flatten()
                assert not bool((ag.ou_x[rest] == want[rest]).any())
                checked += len(rows)
            assert bool((ag.ou_x[56:] == 0).all())
        assert checked >= 56 and (0, True) in tr._sg and (1, True) in tr._sg
        rep = episode_report(tr)
        assert rep["eval_episodes"] > 0 and rep["episodes"] > 0
        assert rep["episodes"] == fin[:56].sum() and rep["eval_episodes"] == fin[56:].sum()
        assert rep["episodes"] + rep["eval_episodes"] == fin.sum()
        assert rep["eval_return_mean"] is not None and rep["eval_length_mean"] <= 20
        assert episode_report(tr)["eval_episodes"] == 0  # cleared
    finally:
        tr.close()


def test_trainer_defaults_report_unchanged(gpu):
    """eval_envs = 0: the env keeps the statistics and episode_report has its three keys only."""
    from f110_gymnasium_ros2_jazzy_amd.train import VectorTrainer, episode_report
    tr = VectorTrainer(16, batch_size=16, memory_size=256, warmup_steps=2, max_episode_steps=5)
    try:
        for _ in range(8):
            tr.step()
        assert tr.train_stats is None and tr.agent.noise_type == "gaussian" and tr.agent.ou_x is None
        assert set(episode_report(tr)) == {"episodes", "episode_return_mean", "episode_length_mean"}
    finally:
        tr.close()
    with pytest.raises(ValueError):
        VectorTrainer(16, eval_envs=16)


def test_main_keeps_best_checkpoint(gpu, monkeypatch, tmp_path, capsys):
    """python -m ...train --noise ou --eval-envs K --ou-reset --save-dir DIR: the report carries the
    eval keys and rank 0 saves DIR/best.pt (the learner's checkpoint) from the eval return."""
    import json
    import sys
    from f110_gymnasium_ros2_jazzy_amd import train
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(sys, "argv", ["train", "--envs-per-gpu", "64", "--steps", "500", "--warmup", "3", "--batch", "64",
                                      "--memory", "4096", "--max-episode-steps", "40", "--noise", "ou", "--eval-envs",
                                      "8", "--ou-reset", "--save-dir", str(tmp_path / "run")])
    train.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["step"] == 500 and line["episodes"] > 0
    assert line["eval_episodes"] > 0 and line["eval_return_mean"] is not None and line["eval_length_mean"] <= 40
    ck = torch.load(tmp_path / "run" / "best.pt", map_location="cpu", weights_only=True)
    assert {"actor", "critic", "actor_target", "critic_target", "global_step"} <= set(ck)
