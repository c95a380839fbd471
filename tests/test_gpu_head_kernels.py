"""The DDPG learner heads (csrc/f110_ddpg.hip, csrc/f110_head_rows.h) called through the C ABI, one
entry at a time, against the float64 references and elementwise bounds of head_refs.py: ragged
shapes (K % 4 != 0, K > 128, one row, partial blocks, a second trip of the finish loops), every
nout, null outputs, dh_mask on every backward, the *_step entries against the separate launches
bit for bit, relu_bwd up to K = 1024, run-to-run determinism and the argument checks.

Every output and scratch buffer is a view into a larger NaN-filled tensor: a write outside it, or
an element an entry should write and does not, fails."""
import ctypes
import functools
import math

import pytest
import torch

import head_refs as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 128, 2), (7, 1, 1), (8, 3, 4), (9, 12, 3), (63, 127, 2), (64, 128, 1), (65, 129, 2), (130, 130, 3),
          (333, 252, 4), (40, 255, 2), (4100, 128, 2), (4100, 255, 1)]
BK = [(B, K) for B, K, _ in SHAPES]
RELU_SHAPES = [(1, 1), (9, 12), (65, 130), (333, 1023), (64, 1024), (4100, 128)]
G = 0.7  # the loss gradient
GAMMA = 0.99
TINY = 2.0 ** -126  # the smallest normal float32
PAD = 64  # guard floats on either side of a view (keeps the view 16-byte aligned)
SCALE, SHIFT = [0.4189, 10.0, 1.0, 2.5], [0.0, 10.0, 0.0, -0.5]


def _lib():
    from f110_gymnasium_ros2_jazzy_amd import _lib as M
    return M, M.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


class Guarded:
    """n floats inside a NaN-filled tensor with PAD floats on either side."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.big = torch.full((self.n + 2 * PAD,), float("nan"), device="cuda")
        self.flat = self.big[PAD:PAD + self.n]
        self.v = self.flat.view(*shape)
        self.bits = self.big.view(torch.int32).clone()

    def check(self, what, written=None):
        """Nothing outside the view changed; no NaN inside (inside flat[:written] for a scratch buffer an
        entry fills only in part)."""
        now = self.big.view(torch.int32)
        assert torch.equal(now[:PAD], self.bits[:PAD]), f"{what}: written below the buffer"
        assert torch.equal(now[PAD + self.n:], self.bits[PAD + self.n:]), f"{what}: written past the buffer"
        inside = self.flat if written is None else self.flat[:written]
        assert not bool(torch.isnan(inside).any()), f"{what}: {int(torch.isnan(inside).sum())} elements not written"
        return self.v


def _mask_like(B, K, g):
    """Mask values of both kinds: > 0 (the smallest normal among them) and <= 0 (-0.0 and 0.0 among
    them); for B >= 3 rows 0..2 put one of each special value into every column (row 1, the second
    row lane of the column sums, is a kept one)."""
    m = torch.randn(B, K, device="cuda", generator=g)
    pick = torch.randint(0, 8, (B, K), device="cuda", generator=g)
    m[pick == 0] = -0.0
    m[pick == 1] = 0.0
    m[pick == 2] = TINY
    if B >= 3:
        m[0], m[1], m[2] = -0.0, TINY, 0.0
    return m


@functools.lru_cache(maxsize=None)
def _inputs(B, K, nout):
    """Post-ReLU h with exact zeros, W ~ 0.5 / sqrt(K), one row scaled to |z| > 10 on every output
    (B >= 7), d in {0, 1}, w in [0.5, 1.5], masks with -0.0 / 0.0 / the smallest normal.  Cached:
    the kernels only read them."""
    g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * K + nout)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = {}
    for tag in ("", "t"):  # the online head and the target head of critic_step
        h = torch.relu(rn(B, K))
        W = rn(nout, K) * (0.5 / math.sqrt(K))
        b = rn(nout) * 0.1
        if B >= 7:
            row = B // 2
            h[row] = rn(K).abs() + 0.1
            zmin = (h[row].double()[None] * W.double()).sum(-1).abs().min()
            h[row] *= float(12.5 / zmin)
            h[0, 0] = 0.0  # an exact zero whatever the draws were
        x["h" + tag], x["W" + tag], x["b" + tag] = h, W, b
    x["mask"] = _mask_like(B, K, g)
    x["dact"] = rn(B, nout)
    x["dact"][torch.rand(B, nout, device="cuda", generator=g) < 0.1] = 0.0
    x["r"] = rn(B)
    x["d"] = (torch.rand(B, device="cuda", generator=g) < 0.3).float()
    if B >= 2:
        x["d"][0], x["d"][1] = 0.0, 1.0
    x["w"] = torch.rand(B, device="cuda", generator=g) + 0.5
    x["y"] = rn(B)
    x["g"] = torch.full((), G, device="cuda")
    x["scale"] = torch.tensor(SCALE[:nout], device="cuda")
    x["shift"] = torch.tensor(SHIFT[:nout], device="cuda")
    # the input conditions, on the float64 reference alone
    z, _ = R.dot(x["h"], x["W"], x["b"])
    sat = (z.abs() > 9.0).any(1)
    assert int(sat.sum()) * 4 < max(B, 4), "a quarter of the rows or more saturate"
    if B >= 7:
        assert bool((z.abs() > 10.0).all(1).any()), "no saturated row"
        assert bool((x["h"] == 0).any()), "h has no exact zero"
    if B >= 8:
        keep = x["mask"] > 0
        assert bool(keep.any(0).all()) and bool((~keep).any(0).all()), "a mask column has one kind of entry only"
        assert bool((x["d"] == 0).any()) and bool((x["d"] == 1).any())
        m = x["mask"]
        assert bool((m == TINY).any()) and bool(((m == 0) & torch.signbit(m)).any()) and \
            bool(((m == 0) & ~torch.signbit(m)).any())
    return x


def _scratch(L, B, K, nout):
    n = L.f110_ddpg_scratch_floats(B, K, nout)
    nbw, nbr = (B + 63) // 64, (B + 7) // 8
    assert n == B * nout + max(nbw * nout * (K + 1), nbr)
    return Guarded(n)


def _check_backward(what, B, K, nout, h, W, mask, dz_dev, dh, dW, db):
    """dh, dW, db (each a Guarded or None) from the dz the kernel wrote."""
    dz_dev = dz_dev.reshape(B, nout)
    if dh is not None:
        ref, bound = R.dh(dz_dev, W, mask)
        got = dh.check(what + " dh")
        R.assert_within(got, ref, bound, what + " dh")
        if mask is not None:
            off = ~(mask > 0)
            assert bool((got[off] == 0).all()) and not bool(torch.signbit(got[off]).any()), what + ": masked dh not +0"
    if dW is not None or db is not None:
        rW, bW, rb, bb = R.wgrad(dz_dev, h)
        if dW is not None:
            R.assert_within(dW.check(what + " dW"), rW, bW, what + " dW")
        if db is not None:
            R.assert_within(db.check(what + " db"), rb, bb, what + " db")


# ---------------------------------------------------------------------- device tanhf --
def test_device_tanh_ulps(gpu):
    """The device tanhf through f110_ddpg_actor_head at K = 1, W = 1, b = 0, scale = 1, shift = 0
    (z = h exactly, act = t): its largest error in ulps of the float64 reference is within the
    figure head_refs.py records, and that figure is no finding (<= 4 ulps)."""
    M, L = _lib()
    small = torch.logspace(-30, -4, 4001, dtype=torch.float64)
    zs = torch.cat([torch.linspace(-12, 12, 120001, dtype=torch.float64), small, -small, torch.zeros(1)])
    h = zs.float().cuda().reshape(-1, 1)
    B = h.shape[0]
    one, zero = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    act, t = Guarded(B, 1), Guarded(B, 1)
    M.check(L.f110_ddpg_actor_head(_p(h), _p(one), _p(zero), _p(one), _p(zero), B, 1, 1, _p(act.v), _p(t.v), _st()),
            "actor_head")
    torch.cuda.synchronize()
    tv, av = t.check("t"), act.check("act")
    assert torch.equal(tv, av)  # 1 * t + 0
    ref = torch.tanh(h.double())
    ulps = (tv.double() - ref).abs() / R.ulp32(ref)
    i = int(ulps.argmax())
    print(f"device tanhf: max {float(ulps.max()):.4f} ulps at z = {float(h.reshape(-1)[i])!r}; "
          f"|z| <= 1e-4: max {float(ulps[h.abs() <= 1e-4].max()):.4f} ulps")
    assert bool((tv[h == 0] == 0).all())
    assert bool((tv.abs() <= 1).all())
    assert float(ulps.max()) <= math.ceil(R.TANH_MEASURED), "larger than the recorded maximum: measure again"
    assert R.TANH_MEASURED <= R.TANH_FINDING_ULPS


# ------------------------------------------------------------------------ actor head --
@pytest.mark.parametrize("B,K,nout", SHAPES)
def test_actor_head_and_backward(gpu, B, K, nout):
    M, L = _lib()
    x = _inputs(B, K, nout)
    h, W, b, scale, shift, dact = x["h"], x["W"], x["b"], x["scale"], x["shift"], x["dact"]
    act, t = Guarded(B, nout), Guarded(B, nout)
    M.check(L.f110_ddpg_actor_head(_p(h), _p(W), _p(b), _p(scale), _p(shift), B, K, nout, _p(act.v), _p(t.v), _st()),
            "actor_head")
    tv, av = t.check("t"), act.check("act")
    tref, tb, z = R.actor_t(h, W, b)
    R.assert_within(tv, tref, tb, "t")
    R.assert_within(av, *R.actor_act(tv, scale, shift), "act")
    sat = z.abs() > 10.0
    assert bool((tv[sat].abs() == 1).all())

    def bwd(mask, want):
        dh = Guarded(B, K) if "dh" in want else None
        dW = Guarded(nout, K) if "dW" in want else None
        db = Guarded(nout) if "db" in want else None
        sc = _scratch(L, B, K, nout)
        M.check(L.f110_ddpg_actor_head_bwd(_p(h), _p(W), _p(tv), _p(scale), _p(dact), B, K, nout,
                                           _p(dh.v) if dh else None, _p(mask), _p(dW.v) if dW else None,
                                           _p(db.v) if db else None, _p(sc.v), _st()), "actor_head_bwd")
        wrote = B * nout + ((B + 63) // 64 * nout * (K + 1) if dW or db else 0)
        sc.check("scratch", written=wrote)
        return sc.flat[:B * nout], dh, dW, db

    for mask in (None, x["mask"]):
        for want in ("dh dW db", "dW db", "dh db", "dh dW", "dh"):
            what = f"actor_bwd[{'mask' if mask is not None else 'no mask'}; {want}]"
            dz, dh, dW, db = bwd(mask, want)
            R.assert_within(dz, *R.actor_dz(dact, scale, tv), what + " dz")
            assert bool((dz.reshape(B, nout)[sat] == 0).all()), "dz of a saturated output is not 0"
            _check_backward(what, B, K, nout, h, W, mask, dz, dh, dW, db)
    a, c = bwd(x["mask"], "dh dW db"), bwd(x["mask"], "dh dW db")
    for u, v in zip(a, c):  # deterministic, bit for bit
        assert torch.equal((u if torch.is_tensor(u) else u.v).view(torch.int32),
                           (v if torch.is_tensor(v) else v.v).view(torch.int32))


# ---------------------------------------------------------------------- critic heads --
def _td_target(M, L, x, B, K, tag="t"):
    y = Guarded(B)
    M.check(L.f110_ddpg_td_target(_p(x["h" + tag]), _p(x["W" + tag][:1]), _p(x["b" + tag][:1]), _p(x["r"]), _p(x["d"]),
                                  GAMMA, B, K, _p(y.v), _st()), "td_target")
    return y.check("y")


def _critic_loss(M, L, x, B, K, y):
    td, loss, sc = Guarded(B), Guarded(1), _scratch(L, B, K, 1)
    M.check(L.f110_ddpg_critic_loss(_p(x["h"]), _p(x["W"][:1]), _p(x["b"][:1]), _p(y), _p(x["w"]), B, K, _p(td.v),
                                    _p(loss.v), _p(sc.v), _st()), "critic_loss")
    nbr = L.f110_ddpg_row_blocks(B)
    assert nbr == (B + 7) // 8
    assert not bool(torch.isnan(sc.flat[B:B + nbr]).any())
    sc.check("critic_loss scratch", written=0)
    return td.check("td"), loss.check("loss"), sc.flat[B:B + nbr]


def _critic_loss_bwd(M, L, x, B, K, td, mask, want):
    dh = Guarded(B, K) if "dh" in want else None
    dW = Guarded(1, K) if "dW" in want else None
    db = Guarded(1) if "db" in want else None
    sc = _scratch(L, B, K, 1)
    M.check(L.f110_ddpg_critic_loss_bwd(_p(x["h"]), _p(x["W"][:1]), _p(td), _p(x["w"]), _p(x["g"]), B, K,
                                        _p(dh.v) if dh else None, _p(mask), _p(dW.v) if dW else None,
                                        _p(db.v) if db else None, _p(sc.v), _st()), "critic_loss_bwd")
    sc.check("critic_loss_bwd scratch", written=B + ((B + 63) // 64 * (K + 1) if dW or db else 0))
    return sc.flat[:B], dh, dW, db


@pytest.mark.parametrize("B,K", BK)
def test_td_target_critic_loss_and_backward(gpu, B, K):
    M, L = _lib()
    x = _inputs(B, K, 1)
    g32 = _f32(GAMMA)
    y = _td_target(M, L, x, B, K)
    R.assert_within(y, *R.td_target(x["ht"], x["Wt"][:1], x["bt"][:1], x["r"], x["d"], g32), "y")
    td, loss, part = _critic_loss(M, L, x, B, K, y)
    R.assert_within(td, *R.td_error(x["h"], x["W"][:1], x["b"][:1], y), "td")
    lref, lb, pref, pb = R.wmse(td, x["w"])
    R.assert_within(loss, lref.reshape(1), lb.reshape(1), "critic loss")
    R.assert_within(part, pref, pb, "critic loss partials")
    for mask, want in ((x["mask"], "dh dW db"), (None, "dW"), (x["mask"], "dh")):
        what = f"critic_loss_bwd[{'mask' if mask is not None else 'no mask'}; {want}]"
        dq, dh, dW, db = _critic_loss_bwd(M, L, x, B, K, td, mask, want)
        R.assert_within(dq, *R.critic_dq(td, x["w"], _f32(G), B), what + " dq")
        _check_backward(what, B, K, 1, x["h"], x["W"][:1], mask, dq, dh, dW, db)
    a = _critic_loss_bwd(M, L, x, B, K, td, x["mask"], "dh dW db")
    c = _critic_loss_bwd(M, L, x, B, K, td, x["mask"], "dh dW db")
    for u, v in zip(a[1:], c[1:]):
        assert torch.equal(u.v.view(torch.int32), v.v.view(torch.int32))


def _q_mean(M, L, x, B, K, sign):
    loss, sc = Guarded(1), _scratch(L, B, K, 1)
    M.check(L.f110_ddpg_q_mean(_p(x["h"]), _p(x["W"][:1]), _p(x["b"][:1]), sign, B, K, _p(loss.v), _p(sc.v), _st()),
            "q_mean")
    nbr = (B + 7) // 8
    sc.check("q_mean scratch", written=0)
    assert not bool(torch.isnan(sc.flat[B:B + nbr]).any())
    return loss.check("loss"), sc.flat[B:B + nbr]


def _q_mean_bwd(M, L, x, B, K, sign, mask, want, h=True):
    dh = Guarded(B, K) if "dh" in want else None
    dW = Guarded(1, K) if "dW" in want else None
    db = Guarded(1) if "db" in want else None
    sc = _scratch(L, B, K, 1)
    M.check(L.f110_ddpg_q_mean_bwd(_p(x["h"]) if h else None, _p(x["W"][:1]), _p(x["g"]), sign, B, K,
                                   _p(dh.v) if dh else None, _p(mask), _p(dW.v) if dW else None,
                                   _p(db.v) if db else None, _p(sc.v), _st()), "q_mean_bwd")
    sc.check("q_mean_bwd scratch", written=B + ((B + 63) // 64 * (K + 1) if dW or db else 0))
    return sc.flat[:B], dh, dW, db


@pytest.mark.parametrize("B,K", BK)
def test_q_mean_and_backward(gpu, B, K):
    M, L = _lib()
    x = _inputs(B, K, 1)
    for sign in (-1.0, 1.0):
        loss, part = _q_mean(M, L, x, B, K, sign)
        lref, lb, pref, pb = R.q_mean(x["h"], x["W"][:1], x["b"][:1], sign)
        R.assert_within(loss, lref.reshape(1), lb.reshape(1), f"q_mean[{sign}]")
        R.assert_within(part, pref, pb, f"q_mean[{sign}] partials")
        for mask, want, h in ((x["mask"], "dh dW db", True), (x["mask"], "dh", False), (None, "db", True)):
            what = f"q_mean_bwd[{sign}; {'mask' if mask is not None else 'no mask'}; {want}]"
            dq, dh, dW, db = _q_mean_bwd(M, L, x, B, K, sign, mask, want, h)
            R.assert_within(dq, *R.mean_dq(sign, _f32(G), B, dq), what + " dq")
            _check_backward(what, B, K, 1, x["h"], x["W"][:1], mask, dq, dh, dW, db)
    a = _q_mean_bwd(M, L, x, B, K, -1.0, x["mask"], "dh dW db")
    c = _q_mean_bwd(M, L, x, B, K, -1.0, x["mask"], "dh dW db")
    for u, v in zip(a[1:], c[1:]):
        assert torch.equal(u.v.view(torch.int32), v.v.view(torch.int32))


# ------------------------------------------------------------------ the *_step entries --
@pytest.mark.parametrize("B,K", BK)
def test_critic_step(gpu, B, K):
    """f110_ddpg_critic_step against float64, and against f110_ddpg_td_target + f110_ddpg_critic_loss +
    f110_ddpg_critic_loss_bwd bit for bit (include/f110.h: "same float operations")."""
    M, L = _lib()
    x = _inputs(B, K, 1)
    nbr = L.f110_ddpg_row_blocks(B)

    def step(dh_on, dq_on):
        td, part = Guarded(B), Guarded(nbr)
        dh, dq = (Guarded(B, K) if dh_on else None), (Guarded(B) if dq_on else None)
        M.check(L.f110_ddpg_critic_step(_p(x["ht"]), _p(x["Wt"][:1]), _p(x["bt"][:1]), _p(x["r"]), _p(x["d"]), GAMMA,
                                        _p(x["h"]), _p(x["W"][:1]), _p(x["b"][:1]), _p(x["w"]), _p(x["g"]), B, K,
                                        _p(td.v), _p(dh.v) if dh else None, _p(x["mask"]), _p(dq.v) if dq else None,
                                        _p(part.v), _st()), "critic_step")
        return td.check("td"), part.check("part"), dh, dq

    td, part, dh, dq = step(True, True)
    yref, yb = R.td_target(x["ht"], x["Wt"][:1], x["bt"][:1], x["r"], x["d"], _f32(GAMMA))
    R.assert_within(td, *R.td_error(x["h"], x["W"][:1], x["b"][:1], yref, yb), "td")
    _, _, pref, pb = R.wmse(td, x["w"])
    R.assert_within(part, pref, pb, "part")
    dqv = dq.check("dq")
    R.assert_within(dqv, *R.critic_dq(td, x["w"], _f32(G), B), "dq")
    _check_backward("critic_step", B, K, 1, x["h"], x["W"][:1], x["mask"], dqv, dh, None, None)
    # the separate launches
    y = _td_target(M, L, x, B, K)
    td_s, _, part_s = _critic_loss(M, L, x, B, K, y)
    dq_s, dh_s, _, _ = _critic_loss_bwd(M, L, x, B, K, td_s, x["mask"], "dh")
    bits = lambda t: t.reshape(-1).view(torch.int32)  # noqa: E731
    assert torch.equal(bits(td), bits(td_s)), "td differs from td_target + critic_loss"
    assert torch.equal(bits(part), bits(part_s)), "part differs from critic_loss's partials"
    assert torch.equal(bits(dqv), bits(dq_s)), "dq differs from critic_loss_bwd"
    assert torch.equal(bits(dh.v), bits(dh_s.check("dh"))), "dh differs from critic_loss_bwd"
    # dh and dq not wanted: td and part all the same
    td2, part2, _, _ = step(False, False)
    assert torch.equal(bits(td2), bits(td)) and torch.equal(bits(part2), bits(part))


@pytest.mark.parametrize("B,K", BK)
def test_q_mean_step(gpu, B, K):
    """f110_ddpg_q_mean_step against float64, and against f110_ddpg_q_mean + f110_ddpg_q_mean_bwd bit
    for bit."""
    M, L = _lib()
    x = _inputs(B, K, 1)
    nbr = L.f110_ddpg_row_blocks(B)
    bits = lambda t: t.reshape(-1).view(torch.int32)  # noqa: E731
    for sign in (-1.0, 1.0):
        part, dh = Guarded(nbr), Guarded(B, K)
        M.check(L.f110_ddpg_q_mean_step(_p(x["h"]), _p(x["W"][:1]), _p(x["b"][:1]), _p(x["g"]), sign, B, K, _p(dh.v),
                                        _p(x["mask"]), _p(part.v), _st()), "q_mean_step")
        _, _, pref, pb = R.q_mean(x["h"], x["W"][:1], x["b"][:1], sign)
        R.assert_within(part.check("part"), pref, pb, "part")
        _, part_s = _q_mean(M, L, x, B, K, sign)
        dq_s, dh_s, _, _ = _q_mean_bwd(M, L, x, B, K, sign, x["mask"], "dh")
        R.assert_within(dq_s, *R.mean_dq(sign, _f32(G), B, dq_s), "dq")
        _check_backward("q_mean_step", B, K, 1, x["h"], x["W"][:1], x["mask"], dq_s, dh, None, None)
        assert torch.equal(bits(part.v), bits(part_s)), "part differs from q_mean's partials"
        assert torch.equal(bits(dh.v), bits(dh_s.check("dh"))), "dh differs from q_mean_bwd"
        part2 = Guarded(nbr)  # dh not wanted
        M.check(L.f110_ddpg_q_mean_step(_p(x["h"]), _p(x["W"][:1]), _p(x["b"][:1]), _p(x["g"]), sign, B, K, None,
                                        None, _p(part2.v), _st()), "q_mean_step")
        assert torch.equal(bits(part2.check("part")), bits(part.v))


# -------------------------------------------------------------------------- relu_bwd --
@pytest.mark.parametrize("B,K", RELU_SHAPES)
def test_relu_bwd(gpu, B, K):
    """gz is gy's bits where y > 0 and +0.0 elsewhere (y: -0.0, 0.0 and the smallest normal among its
    values); db from the gz written; both with db wanted and with db null; twice, bit for bit."""
    M, L = _lib()
    g = torch.Generator(device="cuda").manual_seed(7 * B + K)
    gy = torch.randn(B, K, device="cuda", generator=g)
    gy[torch.rand(B, K, device="cuda", generator=g) < 0.05] = 0.0
    y = _mask_like(B, K, g)
    if B >= 8:
        assert bool((y > 0).any(0).all()) and bool((~(y > 0)).any(0).all())
    n = L.f110_ddpg_relu_bwd_scratch_floats(B, K)
    assert n == (B + 63) // 64 * K
    bits = lambda t: t.reshape(-1).view(torch.int32)  # noqa: E731
    want = torch.where(y > 0, gy, torch.zeros_like(gy))
    outs = []
    for db_on in (True, False, True):
        gz, db, sc = Guarded(B, K), (Guarded(K) if db_on else None), Guarded(n)
        M.check(L.f110_ddpg_relu_bwd(_p(gy), _p(y), B, K, _p(gz.v), _p(db.v) if db else None, _p(sc.v), _st()),
                "relu_bwd")
        gzv = gz.check("gz")
        sc.check("scratch", written=n if db_on else 0)
        assert torch.equal(bits(gzv), bits(want)), "gz is not gy / +0.0 bit for bit"
        if db_on:
            R.assert_within(db.check("db"), *R.relu_db(gzv), "db")
            outs.append(db.v)
    assert torch.equal(bits(outs[0]), bits(outs[1]))


# ------------------------------------------------------------------------ rejections --
def test_head_entries_reject_bad_arguments(gpu):
    """K = 256, nout = 5, B = 0, relu_bwd's K = 1025, q_mean_bwd wanting dW without h and relu_bwd
    wanting db without scratch fail with F110_E_INVALID before any launch (the outputs stay NaN);
    K = 255 and nout = 4 are accepted."""
    M, L = _lib()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    one, g = torch.ones(4, device="cuda"), torch.full((), G, device="cuda")
    out = [Guarded(8, 5), Guarded(8, 5), Guarded(1), Guarded(8, 1025), Guarded(1025), Guarded(1, 256)]
    act, t, loss, gz, db, dW = out
    sc = z(1 << 16)

    keep = []  # the arguments stay allocated until the launches are done

    def actor(B, K, nout):
        a = [z(max(B, 1), K), z(nout, K), z(nout), z(nout) + 1, z(nout)]
        keep.extend(a)
        return L.f110_ddpg_actor_head(*[_p(v) for v in a], B, K, nout, _p(act.v), _p(t.v), _st())

    def qm(B, K):
        a = [z(max(B, 1), K), z(1, K), z(1)]
        keep.extend(a)
        return L.f110_ddpg_q_mean(*[_p(v) for v in a], -1.0, B, K, _p(loss.v), _p(sc), _st())

    assert L.f110_ddpg_scratch_floats(8, 256, 1) == -1 and L.f110_ddpg_scratch_floats(8, 16, 5) == -1
    assert L.f110_ddpg_scratch_floats(0, 16, 1) == -1 and L.f110_ddpg_row_blocks(0) == -1
    assert L.f110_ddpg_relu_bwd_scratch_floats(8, 1025) == -1 and L.f110_ddpg_relu_bwd_scratch_floats(0, 8) == -1
    for rc in (actor(8, 256, 2), actor(8, 16, 5), actor(0, 16, 2), qm(8, 256), qm(0, 16),
               L.f110_ddpg_actor_head_bwd(_p(z(8, 16)), _p(z(5, 16)), _p(z(8, 5)), _p(one), _p(z(8, 5)), 8, 16, 5,
                                          None, None, _p(dW.v), None, _p(sc), _st()),
               L.f110_ddpg_critic_step(_p(z(8, 256)), _p(z(1, 256)), _p(z(1)), _p(z(8)), _p(z(8)), GAMMA,
                                       _p(z(8, 256)), _p(z(1, 256)), _p(z(1)), _p(one), _p(g), 8, 256, _p(act.v), None,
                                       None, None, _p(loss.v), _st()),
               L.f110_ddpg_q_mean_step(_p(z(8, 16)), _p(z(1, 16)), _p(z(1)), _p(g), -1.0, 0, 16, None, None,
                                       _p(loss.v), _st()),
               L.f110_ddpg_relu_bwd(_p(z(8, 1025)), _p(z(8, 1025)), 8, 1025, _p(gz.v), _p(db.v), _p(sc), _st()),
               L.f110_ddpg_relu_bwd(_p(z(8, 16)), _p(z(8, 16)), 0, 16, _p(gz.v), None, None, _st()),
               L.f110_ddpg_relu_bwd(_p(z(8, 16)), _p(z(8, 16)), 8, 16, _p(gz.v), _p(db.v), None, _st()),
               L.f110_ddpg_q_mean_bwd(None, _p(z(1, 16)), _p(g), -1.0, 8, 16, None, None, _p(dW.v), None, _p(sc),
                                      _st()),
               L.f110_ddpg_q_mean_bwd(None, _p(z(1, 16)), _p(g), -1.0, 8, 16, None, None, None, _p(db.v), _p(sc),
                                      _st())):
        assert rc < 0
        with pytest.raises(M.F110Error):
            M.check(rc, "head entry")
    torch.cuda.synchronize()
    for o in out:  # nothing was launched
        assert bool(torch.isnan(o.big).all())
    assert L.f110_ddpg_scratch_floats(8, 255, 4) == 8 * 4 + 4 * 256
    assert actor(8, 255, 4) == 0 and qm(8, 255) == 0
    torch.cuda.synchronize()
    assert bool((act.flat[:32] == 0).all()) and bool((t.flat[:32] == 0).all()) and float(loss.v) == 0.0
