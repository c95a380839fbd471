"""What tests/test_scan_obs_host.py and tests/test_gpu_scan_obs.py share: a NumPy restatement of the
scan observation's row rule (include/f110.h, "scan observation"), outside the library, the case
list and the row generator."""
import numpy as np

# (B, K, F, S): the default shape, ragged bins with D = 5, identity pooling, a tiny row, one bin and
# the deepest stack at stride 1, and the identity over the whole 1080-beam row
CASES = ((1080, 108, 1, 1), (1080, 7, 3, 2), (67, 67, 2, 1), (5, 3, 1, 1), (1080, 1, 8, 1), (1080, 1080, 1, 1))
REDUCES = ("min", "mean")
# The deepest ring F <= 8 and S <= 16 reach: D = 31 (D = 32 would need (F-1)*S = 31, a prime, so
# S = 31); F = 3, S = 16 gives D = 33, which is refused.
DEEP = (40, 6, 3, 15)
ENVS_HOST = (1, 3, 65)
ENVS_GPU = (1, 3, 65, 130)  # one wave, an odd tail of the 4-env block, more than one block, a ragged last block


def depth(F, S):
    return (F - 1) * S + 1


def width(K, F, M, T, keep_mid=True):
    return F * K + (M if keep_mid else 0) + T


def pool(scans, K, reduce):
    """The K pooled values of every row of scans [N, B] (all rows at once, one beam at a time):
    float32 throughout, the mean's sum in ascending beam order from the first beam's value."""
    N, B = scans.shape
    out = np.empty((N, K), np.float32)
    for j in range(K):
        lo, hi = (j * B) // K, ((j + 1) * B) // K
        acc = scans[:, lo].astype(np.float32)
        for b in range(lo + 1, hi):
            acc = np.fmin(acc, scans[:, b]) if reduce == "min" else (acc + scans[:, b]).astype(np.float32)
        out[:, j] = acc if reduce == "min" else acc / np.float32(hi - lo)
    return out


def fresh(N, K, F, S):
    return {"ring": np.zeros((N, depth(F, S), K), np.float32), "head": np.full(N, -1, np.int32)}


def push(state, rows, B, M, T, K, F, S, reduce="min", keep_mid=True, reset=None):
    """One push of every env; ``state`` (fresh's layout) is updated in place.  Returns the rows."""
    ring, head = state["ring"], state["head"]
    N, D = head.shape[0], depth(F, S)
    out = np.empty((N, width(K, F, M, T, keep_mid)), np.float32)
    pooled = pool(rows[:, :B], K, reduce)
    for e in range(N):
        p = pooled[e]
        if head[e] < 0 or (reset is not None and reset[e]):
            ring[e, :] = p
            head[e] = 0
        else:
            head[e] = (head[e] + 1) % D
            ring[e, head[e]] = p
        for j in range(F):
            out[e, j * K:(j + 1) * K] = ring[e, (head[e] - j * S) % D]
        rest = rows[e, B:B + M + T] if keep_mid else rows[e, B + M:B + M + T]
        out[e, F * K:] = rest
    return out


def rows_for(rng, N, B, M, T, stride=None):
    """Full rows [N, B + M + T] as a view of a wider array when stride is given: ranges in [0, 1),
    those of every other env on a 1/64 grid (ties inside a bin), the other columns of any sign."""
    W = B + M + T
    base = rng.random((N, stride or W), dtype=np.float32)
    base[::2, :B] = np.round(base[::2, :B] * np.float32(64.0)) / np.float32(64.0)  # every other env: coarse values
    base[:, B:W] = (base[:, B:W] - np.float32(0.5)) * np.float32(40.0)
    return base[:, :W]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
