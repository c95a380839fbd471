"""Shared by the sensor-randomization tests (CPU and GPU): the shapes, the active ranges, seeded
rows, and an independent NumPy restatement of the row rule of include/f110.h ("sensor
randomization"): Philox4x32-10 in uint64 arithmetic, the parameter draw, the counter rule and the
per-column rule in float32, one operation at a time (NumPy never fuses a multiply and an add)."""
import numpy as np

F = np.float32
U = np.uint64
M32 = U(0xFFFFFFFF)
PARAM_TAG, DRAW_TAG = 0x5E250, 0x5E251
NAMES = ("scale", "noise_abs", "noise_rel", "dropout", "blackout", "quant", "pose_xy", "pose_theta")
IDENTITY = {n: (1.0, 1.0) if n == "scale" else (0.0, 0.0) for n in NAMES}
RANGE_MAX = 30.0

BEAMS = (1, 63, 64, 65, 130, 1080)  # below, at and above one wave's 64 columns; more than two passes; the env's own
MIDS = (4, 8)
TAILS = (0, 5)
N_ENVS, ENV_OFFSET, SEED = 3, 7, 0x1234_5678_9ABC_DEF0
APPLIES, RESET_AT, RESET_ENV = 6, 2, 1  # six applies, a reset flag for one env at the third


def active(B):
    """Ranges with every parameter active (blackout bounded by the B beams)."""
    return dict(scale=(0.97, 1.03), noise_abs=(0.005, 0.05), noise_rel=(0.001, 0.02), dropout=(0.01, 0.1),
                blackout=(min(B, 1), min(B, 40)), quant=(0.01, 0.05), pose_xy=(0.01, 0.05), pose_theta=(0.005, 0.3))


def rows_for(rng, N, B, M, T, stride=None):
    """float32 [N, B + M + T] rows like the env's: ranges in [0, 1] (some exactly 0 and 1), pose
    groups (x, y in +-20 m, theta in [-pi, pi] with some at the ends, collision 0 / 1), a tail of
    normals.  stride: the rows are a view into a wider array."""
    W = B + M + T
    full = np.full((N, stride or W), F(-7.0))
    rows = full[:, :W]
    r = rng.random((N, B)).astype(F)
    r[rng.random((N, B)) < 0.05] = F(1.0)
    r[rng.random((N, B)) < 0.02] = F(0.0)
    rows[:, :B] = r
    for g in range(M // 4):
        c = B + 4 * g
        rows[:, c:c + 2] = rng.uniform(-20, 20, (N, 2)).astype(F)
        th = rng.uniform(-np.pi, np.pi, N).astype(F)
        th[rng.random(N) < 0.4] = F(np.pi) * F(1 if g % 2 else -1)
        rows[:, c + 2] = th
        rows[:, c + 3] = (rng.random(N) < 0.3).astype(F)
    rows[:, B + M:] = rng.normal(size=(N, T)).astype(F)
    return rows


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement --------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: the counter words as uint64 arrays holding 32-bit values (they broadcast), the
    key two Python ints.  Returns four uint64 arrays of 32-bit values."""
    x, y, z, w = (a.copy() for a in np.broadcast_arrays(*(np.asarray(v, dtype=U) for v in (c0, c1, c2, c3))))
    for _ in range(10):
        p0 = U(0xD2511F53) * x
        p1 = U(0xCD9E8D57) * z
        x, y, z, w = (p1 >> U(32)) ^ y ^ U(k0), p1 & M32, (p0 >> U(32)) ^ w ^ U(k1), p0 & M32
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return x, y, z, w


def key(seed, gid):
    return (seed ^ gid) & 0xFFFFFFFF, ((seed >> 32) ^ (gid >> 32) ^ 0xA5A5A5A5) & 0xFFFFFFFF


def uniform(pair, word):
    lo, hi = F(pair[0]), F(pair[1])
    u = F(int(word) >> 8) * F(2.0 ** -24)
    return F(lo + F(u * F(hi - lo)))


def below(word, n):
    return (int(word) * int(n)) >> 32


def draw_row(seed, gid, episode, ranges, B, range_max):
    """The ten floats of f110_sensor_arrays' parameter row."""
    k0, k1 = key(seed, gid)
    a, b, c = ([int(v) for v in philox(j, 0, PARAM_TAG, episode, k0, k1)] for j in range(3))
    rm = F(range_max)
    p = F(uniform(ranges["dropout"], a[3]))
    w_lo, w_hi = int(ranges["blackout"][0]), int(ranges["blackout"][1])
    w = w_lo + below(b[0], w_hi - w_lo + 1)
    return np.array([uniform(ranges["scale"], a[0]), F(uniform(ranges["noise_abs"], a[1]) / rm),
                     uniform(ranges["noise_rel"], a[2]), p, F(w), F(below(b[1], B - w + 1)),
                     F(uniform(ranges["quant"], b[2]) / rm), uniform(ranges["pose_xy"], b[3]),
                     uniform(ranges["pose_theta"], c[0]), F(int(F(p * F(16777216.0))))], dtype=F)


def normals(x, y, z):
    s = np.zeros(x.shape, np.int64)
    for word in (x, y, z):
        for i in range(4):
            s += ((word >> U(8 * i)) & U(0xFF)).astype(np.int64)
    return (s - 1530).astype(F) * F(1.0 / 256.0)


def fresh(N):
    return {"params": np.zeros((N, 10), F), "episode": np.full(N, -1, np.int32), "step": np.zeros(N, np.int32)}


def full_ranges(ranges):
    return {**IDENTITY, **{k: (v, v) if np.isscalar(v) else tuple(v) for k, v in ranges.items()}}


def apply(state, rows, B, M, T, ranges, range_max=RANGE_MAX, seed=SEED, env_offset=0, mask=None, reset=None):
    """One apply of every env; state (fresh's layout) is updated in place.  Returns a new array."""
    ranges = full_ranges(ranges)
    N = rows.shape[0]
    out = np.array(rows[:, :B + M + T], dtype=F)  # the collision columns and the tail: carried through
    for e in range(N):
        gid = env_offset + e
        ep, st = int(state["episode"][e]), int(state["step"][e])
        if ep < 0 or (reset is not None and reset[e]):
            ep, st = (ep + 1) & 0x7FFFFFFF, 0
            state["params"][e] = draw_row(seed, gid, ep, ranges, B, range_max)
        else:
            st = (st + 1) & 0xFFFFFFFF
        state["episode"][e], state["step"][e] = ep, np.uint32(st).astype(np.int32)
        if mask is not None and not mask[e]:
            continue
        scale, na, nr, _, bw, bs, q, sxy, sth, thr = state["params"][e]
        k0, k1 = key(seed, gid)
        x, y, z, w = philox(np.arange(B + M, dtype=U), st, DRAW_TAG, ep, k0, k1)
        zn, bits = normals(x, y, z), w >> U(8)
        d = out[e, :B] * scale
        if na > 0 or nr > 0:
            d = d + zn[:B] * (na + nr * d)
        if q > 0:
            d = q * np.rint(d / q)
        d = np.where(bits[:B] < U(int(thr)), F(1.0), d)
        b = np.arange(B)
        d = np.where((b >= int(bs)) & (b < int(bs) + int(bw)), F(0.0), d)
        d = np.where(d < 0, F(0.0), np.where(d > 1, F(1.0), d))
        assert d.dtype == F
        out[e, :B] = d
        for m in range(M):
            v, c = out[e, B + m], m % 4
            if c < 2 and sxy > 0:
                out[e, B + m] = v + zn[B + m] * sxy
            elif c == 2 and sth > 0:
                t = F(v + zn[B + m] * sth)
                pi, two_pi = F(np.pi), F(2 * np.pi)
                out[e, B + m] = t - two_pi if t > pi else (t + two_pi if t < -pi else t)
    return out
