"""Shared by test_gpu_head_kernels.py and test_gpu_adam.py: float64 torch references of every stage
of the DDPG learner heads (csrc/f110_ddpg.hip, csrc/f110_head_rows.h) and of the flat Adam step
(csrc/f110_adam.hip), each with an elementwise error bound, and the helper that asserts one.

Every stage is evaluated in float64 on the float32 values that stage actually read (dW from the dz
the kernel wrote, dz from the td it wrote ...), so each bound is that of one short expression or one
sum: err <= gamma * absref elementwise, no absolute floor (absref == 0 asks for an exact 0).
u = 2**-24 is the float32 unit roundoff; the operation counts are read off the kernel source and
stated at each rule.

Device tanhf: measured by test_gpu_head_kernels.py::test_device_tanh_ulps (f110_ddpg_actor_head at
K = 1, W = 1, b = 0, scale = 1, shift = 0, so z = h exactly; 120001 values over [-12, 12] and 4001
values of either sign in [1e-30, 1e-4], against float64 tanh in ulps of the reference).  Measured
maximum on an MI355X (gfx950, ROCm's ocml): 1.1364 ulps, at z = -0.6424000263214111; 0.0458 ulps
over |z| <= 1e-4.  The actor tests allow TANH_ULPS = ceil(measured) + 1 = 3 ulps.
"""
import math

import torch

U = 2.0 ** -24
GAMMA_DOT = 2e-6  # the learner-GEMM constant; here also worst case: <= 8 fma per lane, 5 tree levels, the bias: 14 u
TANH_MEASURED = 1.1364  # ulps, see the module docstring
TANH_ULPS = math.ceil(TANH_MEASURED) + 1
TANH_FINDING_ULPS = 4  # a measured maximum above this is a finding, not a wider allowance
ROWS_PER_BLOCK = 8  # kRowsPerBlock: rows (half-waves) per block of the row kernels
W_ROWS = 64  # kWRows: rows per block of the weight-gradient and relu_bwd passes


def d(x):
    return x.detach().double()


def ulp32(x):
    """The float32 spacing at |x| (x float64; at least the smallest normal's)."""
    _, e = torch.frexp(x.abs())  # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e.clamp_min(-125) - 24)


def assert_within(got, ref, bound, what):
    """err <= bound elementwise (a NaN fails); prints and returns max err / bound over bound > 0."""
    got, ref, bound = d(got).reshape(-1), ref.reshape(-1), bound.reshape(-1)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}")
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.where(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at flat index {i}: "
                             f"got {got[i].item()!r} ref {ref[i].item()!r} err {err[i].item():.3e} "
                             f"bound {bound[i].item():.3e}; max err / bound {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------ the row dot product --
def dot(h, W, b):
    """z = h W^T + b [B][nout] and its bound GAMMA_DOT (|h| |W|^T + |b|) (row_dot_of)."""
    h, W, b = d(h), d(W), d(b)
    z = (h[:, None, :] * W[None]).sum(-1) + b
    a = (h[:, None, :] * W[None]).abs().sum(-1) + b.abs()
    return z, GAMMA_DOT * a


# ------------------------------------------------------------------------- actor head --
def actor_t(h, W, b, tanh_ulps=TANH_ULPS):
    """t = tanh(z): the z bound times tanh's slope (1 - tanh^2, taken at the point of z's interval
    nearest 0, where it is largest), plus tanh_ulps float32 ulps of the reference."""
    z, zb = dot(h, W, b)
    t = torch.tanh(z)
    slope = 1.0 - torch.tanh((z.abs() - zb).clamp_min(0.0)) ** 2
    return t, zb * slope + tanh_ulps * ulp32(t), z


def actor_act(t, scale, shift):
    """act = scale * t + shift from the t the kernel wrote: 2 operations (mul, add; no FMA) -> 3 u."""
    st = d(scale) * d(t)
    return st + d(shift), 3 * U * (st.abs() + d(shift).abs())


def actor_dz(dact, scale, t):
    """dz = (dact * scale) * (1 - t * t): 4 operations (mul, mul, sub, mul) -> 5 u over the terms
    |dact scale| and |dact scale t^2| of the expanded product."""
    a, t = d(dact) * d(scale), d(t)
    return a * (1.0 - t * t), 5 * U * a.abs() * (1.0 + t * t)


# ---------------------------------------------------------------- the backward's sums --
def dh(dz, W, mask):
    """dh = dz W where mask > 0 (all of it for mask None), else +0: nout fma from 0 -> (nout + 1) u."""
    dz, W = d(dz), d(W)
    ref = (dz[:, :, None] * W[None]).sum(1)
    a = (dz[:, :, None] * W[None]).abs().sum(1)
    if mask is not None:
        keep = (mask > 0).double()
        ref, a = ref * keep, a * keep
    return ref, (dz.shape[1] + 1) * U * a


def gamma_w(B):
    """k_head_wgrad / k_relu_bwd then k_wgrad_finish / k_colsum_finish: a block adds at most
    min(B, 64) rows into one element (fma chain per row lane, then the lanes in LDS), the finish adds
    ceil(nblk / 64) partials per lane and 6 shuffle levels; + 2."""
    nblk = (B + W_ROWS - 1) // W_ROWS
    return (min(B, W_ROWS) + (nblk + 63) // 64 + 8) * U


def wgrad(dz, h):
    """dW = dz^T h [nout][K] over |dz|^T |h|, db = sum_rows dz [nout] over sum |dz|; gamma_w(B)."""
    dz, h = d(dz), d(h)
    g = gamma_w(dz.shape[0])
    p = dz[:, :, None] * h[:, None, :]
    return p.sum(0), g * p.abs().sum(0), dz.sum(0), g * dz.abs().sum(0)


# ------------------------------------------------------------------------ critic heads --
def td_target(h, W, b, r, dn, gamma):
    """y = r + (gamma * (1 - d)) * z: 4 operations (sub, mul, mul, add) -> 5 u over |r| + |gd z|, plus
    the z bound times |gd|.  gamma: the float32 the entry receives."""
    z, zb = dot(h, W, b)
    z, zb = z[:, 0], zb[:, 0]
    gd = gamma * (1.0 - d(dn))
    y = d(r) + gd * z
    return y, zb * gd.abs() + 5 * U * (d(r).abs() + gd.abs() * (z.abs() + zb))


def td_error(h, W, b, y, yb=None):
    """td = y - z: 1 operation -> 2 u over |y| + |z|, plus the z bound (and y's, where y is not an
    input: critic_step)."""
    z, zb = dot(h, W, b)
    z, zb = z[:, 0], zb[:, 0]
    y = d(y)
    if yb is None:
        yb = torch.zeros_like(y)
    return y - z, yb + zb + 2 * U * (y.abs() + yb + z.abs() + zb)


def block_sums(term):
    """The per-block partials of a row kernel (8 rows per block) and of |term|."""
    n = (term.numel() + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK * ROWS_PER_BLOCK
    t = torch.zeros(n, dtype=torch.float64, device=term.device)
    t[:term.numel()] = term
    t = t.reshape(-1, ROWS_PER_BLOCK)
    return t.sum(1), t.abs().sum(1)


def wmse(td, w):
    """loss = mean(w * (td * td)) from the td the kernel wrote, and the block partials of its terms:
    2 roundings per term, then the block, wave and finish sums (about 25 roundings at B <= 4200):
    GAMMA_DOT over mean |term| (sum |term| for a partial)."""
    term = d(w) * (d(td) * d(td))
    part, apart = block_sums(term)
    return term.mean(), GAMMA_DOT * term.abs().mean(), part, GAMMA_DOT * apart


def critic_dq(td, w, g, B):
    """dq = -(((g / B) * w) * (2 * td)): 4 operations (div, mul, the exact doubling, mul) -> 5 u |dq|."""
    dq = -(((float(g) / B) * d(w)) * (2.0 * d(td)))
    return dq, 5 * U * dq.abs()


def mean_dq(sign, g, B, like):
    """dq = sign * (g / B) for every row: 2 operations -> 3 u |dq|."""
    dq = torch.full_like(d(like), sign * (float(g) / B))
    return dq, 3 * U * dq.abs()


def q_mean(h, W, b, sign):
    """loss = sign * mean(z), and the block partials of z: every z within its own bound, then the sums
    with GAMMA_DOT over mean |z| (sum |z| for a partial)."""
    z, zb = dot(h, W, b)
    z, zb = z[:, 0], zb[:, 0]
    part, apart = block_sums(z)
    pzb, _ = block_sums(zb)
    return (sign * z.mean(), zb.mean() + GAMMA_DOT * (z.abs() + zb).mean(), part, pzb + GAMMA_DOT * (apart + pzb))


# ---------------------------------------------------------------------------- relu_bwd --
def relu_db(gz):
    """db = sum_rows gz from the gz the kernel wrote: gamma_w(B) over sum |gz|."""
    gz = d(gz)
    return gz.sum(0), gamma_w(gz.shape[0]) * gz.abs().sum(0)


# -------------------------------------------------------------------------------- Adam --
def adam_moments(m, v, g, beta1, beta2):
    """m' = m + (1 - b1)(g - m): 3 operations and the rounded constant -> 4 u (|m| + w1 (|g| + |m|)).
    v' = v b2 + ((1 - b2) g) g: 4 operations and two rounded constants -> 6 u (b2 |v| + w2 g^2).
    From the copies taken before the launch, with the exact double constants."""
    m, v, g = d(m), d(v), d(g)
    w1, w2 = 1.0 - beta1, 1.0 - beta2
    return (m + w1 * (g - m), 4 * U * (m.abs() + w1 * (g.abs() + m.abs())),
            v * beta2 + (w2 * g) * g, 6 * U * (beta2 * v.abs() + w2 * g * g))


def adam_param(p, m1, v1, t, lr, beta1, beta2, eps):
    """p' = p + (-lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)) from the m', v' the kernel wrote and
    the step t it ran at: sqrt, div, add, div, mul and the three rounded constants (sqrt(bc2), eps,
    lr / bc1) -> 8 roundings of the update, bounded by 10 u |update|; the last add u |p'|."""
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    upd = (-lr / bc1) * (d(m1) / (d(v1).sqrt() / math.sqrt(bc2) + eps))
    p1 = d(p) + upd
    return p1, U * p1.abs() + 10 * U * upd.abs()


def adam_target(q, p1, tau):
    """q' = q + tau (p' - q) from the p' the kernel wrote: 3 operations and the rounded tau ->
    4 u (|q| + tau (|p'| + |q|))."""
    q, p1 = d(q), d(p1)
    return q + tau * (p1 - q), 4 * U * (q.abs() + tau * (p1.abs() + q.abs()))
