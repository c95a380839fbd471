"""The replay sampler's radix select and tie break (k_keys, k_hist x3, k_count, k_place, k_finish
of f110_replay.hip) on keys the test chooses (f110_replay_select_keys), and its production and
with-replacement paths, against the NumPy model of the selection (replay_oracle.select_model: the
B smallest by (key, index), in index order) and PEROracle's float64 weights.

Indices must match the model exactly, weights to rtol 2e-6 (test_gpu_replay's bar).  Rows are 4 + 2
floats, so the largest ring is a few MB.  The rings cover the launch geometry (replay_grid =
ceil(capacity / 1024) clamped to [1, 1024]; k_keys packs 4 streaming blocks into one):
  300            one block
  5000           grid 5: a partly filled k_keys block, grid % 4 != 0
  8192           grid 8: batch == length == the largest batch
  20000          grid 20: the 8 histogram copies wrap
  2^20 + 4096    the grid clamped at 1024
each full and partly filled, with lengths that are no multiple of the grid and one far below it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, A = 4, 2
MAX_BATCH = 8192            # kReplayMaxBatch
TIE_CAP = 4096              # kTieCap
KEY_MAX = 0x7F800000        # the largest pattern k_keys produces (+inf)
BIG = (1 << 20) + 4096
RINGS = [(300, 300), (300, 211), (5000, 5000), (5000, 4099), (5000, 4096), (8192, 8192), (20000, 20000),
         (20000, 12347), (20000, 300), (BIG, BIG), (BIG, 700001)]  # (capacity, stored rows)
RING_IDS = [f"{c}-{n}" for c, n in RINGS]
BETA = 0.4


def _fill(cap, n, seed=0):
    """A ring of `cap` rows holding `n`, with unequal priorities, and the oracle in the same state."""
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    from replay_oracle import PEROracle
    rb = DeviceReplayBuffer(buffer_size=cap, batch_size=MAX_BATCH, obs_dim=D, act_dim=A, device=0)
    prio = np.random.default_rng(seed + cap + n).uniform(0.01, 10.0, n).astype(np.float32)
    z = torch.zeros(n, D, device="cuda")
    rb.add(z, z[:, :A], z[:, 0], z, priority=torch.from_numpy(prio))
    o = PEROracle(cap, MAX_BATCH, alpha=0.6)
    o.prio[:n] = prio  # add(priority=p) stores clip(p, 1e-8, f32 max): p itself here
    o.length, o.next_idx = n, n % cap
    assert len(rb) == n
    return rb, o


@pytest.fixture(scope="module")
def rings(gpu):
    cache = {}

    def get(cap, n):
        if (cap, n) not in cache:
            cache[cap, n] = _fill(cap, n)
        return cache[cap, n]
    yield get
    for rb, _ in cache.values():
        rb.close()


def _distinct(rng, lo, hi, k):
    """k distinct integers in [lo, hi), ascending (random gaps)."""
    if k == 0:
        return np.zeros(0, np.int64)
    g = (hi - lo) // k
    assert g >= 1
    return lo + np.cumsum(rng.integers(1, g + 1, k)) - 1


def _distinct_keys(rng, n):
    return rng.permutation(_distinct(rng, 0, KEY_MAX + 1, n)).astype(np.uint32)


def _check_select(rb, o, keys, B, beta=BETA):
    """One select over `keys`: indices == the model, weights == the oracle's, and the header's
    threshold, rows below it and ties still to take."""
    from replay_oracle import select_model
    keys = np.asarray(keys, np.uint32)
    assert keys.shape == (o.length,) and int(keys.max()) <= KEY_MAX
    idx, w = rb.select_keys(torch.from_numpy(keys), beta, B)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    ref = select_model(keys, B)
    np.testing.assert_array_equal(idx, ref, err_msg=f"len {o.length} B {B}")
    np.testing.assert_allclose(w, o.weights(ref, beta), rtol=2e-6)
    T = np.partition(keys, B - 1)[B - 1]
    n_lt = int((keys < T).sum())
    st = rb.select_state()
    assert (st["prefix"], st["n_lt"], st["kleft"]) == (int(T), n_lt, B - n_lt)
    return idx


@pytest.mark.parametrize("cap,n", RINGS, ids=RING_IDS)
def test_select_distinct_keys(rings, cap, n):
    """Distinct keys spread over every top digit: B around the wave size, a block, a full batch,
    and the whole ring where it fits a batch."""
    rb, o = rings(cap, n)
    keys = _distinct_keys(np.random.default_rng(n), n)
    for B in (1, 2, 63, 64, 65, 256, 4096, n):
        if B <= min(n, MAX_BATCH):
            _check_select(rb, o, keys, B)


# (last key of a bin, first key of the next) at digit 0 (twice), 1, 2 and 3: the lower digits of
# the first are all 0xFF, of the second all 0
BOUNDARIES = [(0x00FFFFFF, 0), (0x3EFFFFFF, 0), (0x3F7FFFFF, 1), (0x3F8000FF, 2), (0x3F800010, 3)]


@pytest.mark.parametrize("cap,n", RINGS, ids=RING_IDS)
def test_select_digit_boundaries(rings, cap, n):
    """The B-th smallest key is the last key of a digit's bin (kleft == the bin's cumulative
    count at that digit), then the first of the next bin (kleft == 1 there), for each of the four
    digits; 40 consecutive keys lie on either side of the boundary, the other rows far from it."""
    rb, o = rings(cap, n)
    rng = np.random.default_rng(cap + n)
    m = 40
    n_below = min(n // 4, 1000)
    for lo_key, digit in BOUNDARIES:
        hi_key = lo_key + 1
        shift = 24 - 8 * digit
        assert (lo_key >> shift) + 1 == hi_key >> shift and hi_key & ((1 << shift) - 1) == 0
        keys = np.concatenate([_distinct(rng, 0, lo_key - m, n_below), lo_key - np.arange(m), hi_key + np.arange(m),
                               _distinct(rng, hi_key + m, KEY_MAX + 1, n - n_below - 2 * m)])
        keys = rng.permutation(keys).astype(np.uint32)
        c = n_below + m  # keys <= lo_key
        for B in (c, c + 1):
            _check_select(rb, o, keys, B)
            assert rb.select_state()["prefix"] == (lo_key if B == c else hi_key)


def test_select_extreme_keys(rings):
    """The patterns 0 and 0x7F800000 among the keys: selected first and last."""
    rb, o = rings(5000, 4099)
    rng = np.random.default_rng(5)
    keys = _distinct_keys(rng, 4099)
    keys[keys == 0] = 1
    keys[keys == KEY_MAX] = KEY_MAX - 1
    keys[[1234, 77]] = 0, KEY_MAX
    assert _check_select(rb, o, keys, 1).tolist() == [1234]
    _check_select(rb, o, keys, 4098)  # all but the largest
    _check_select(rb, o, keys, 4099)
    assert rb.select_state()["prefix"] == KEY_MAX


def _tie_keys(rng, n, n_tie, n_below, T=0x3F000000):
    """n_tie keys equal to T on random rows, the first and the last row among them; n_below
    distinct keys below T and the rest above, interleaved with them."""
    rows = rng.permutation(np.arange(1, n - 1))
    tie = np.concatenate([[0, n - 1], rows[:n_tie - 2]])
    rest = rows[n_tie - 2:]
    keys = np.empty(n, np.uint32)
    keys[tie] = T
    keys[rest[:n_below]] = _distinct(rng, 0, T, n_below)
    keys[rest[n_below:]] = _distinct(rng, T + 1, KEY_MAX + 1, rest.size - n_below)
    return keys


@pytest.mark.parametrize("cap,n", RINGS, ids=RING_IDS)
def test_select_ties_at_threshold(rings, cap, n):
    """n_tie keys equal to the threshold, of which the `need` lowest indices are taken and merged
    into the rows below the threshold in index order."""
    rb, o = rings(cap, n)
    rng = np.random.default_rng(2 * cap + n)
    ran = 0
    for n_tie in (2, 65, TIE_CAP):
        n_below = min(500, (n - n_tie) // 2)
        if n_below < 10:
            continue
        for need in (1, 2, 64):
            if need > n_tie:
                continue
            keys = _tie_keys(rng, n, n_tie, n_below)
            idx = _check_select(rb, o, keys, n_below + need)
            assert idx[0] == 0 and (idx[-1] == n - 1) == (need == n_tie)
            ran += 1
    assert ran >= 5
    assert rb.tie_overflows() == 0


@pytest.mark.parametrize("cap,n", [(c, n) for c, n in RINGS if n <= TIE_CAP],
                         ids=[i for i, (c, n) in zip(RING_IDS, RINGS) if n <= TIE_CAP])
def test_select_all_keys_equal(rings, cap, n):
    """Every key equal (up to kTieCap of them): rows 0 .. B-1."""
    rb, o = rings(cap, n)
    for key in (0x3F800000, 0, KEY_MAX):
        for B in (1, 2, 64):
            idx = _check_select(rb, o, np.full(n, key, np.uint32), B)
            np.testing.assert_array_equal(idx, np.arange(B))
    assert rb.tie_overflows() == 0


def _check_sample(rb, o, B, beta=BETA):
    """An ordinary sample(): idx == the model's selection of the keys it drew, weights == the
    oracle's; the keys are float32(e / w_i) for an e in (0, 37] (-log of a uniform in [2^-53, 1));
    den == the float64 sum of the sampling weights."""
    from replay_oracle import select_model
    n = o.length
    idx, _, w = rb.sample(beta=beta, batch_size=B, gather=False)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    keys = rb.keys().cpu().numpy()[:n]
    ref = select_model(keys, B)
    np.testing.assert_array_equal(idx, ref)
    np.testing.assert_allclose(w, o.weights(ref, beta), rtol=2e-6)
    wt = rb.sampling_weights().cpu().numpy()[:n]
    np.testing.assert_allclose(wt, np.power(o.prio[:n] + np.float32(o.eps), o.alpha, dtype=np.float64), rtol=1e-14)
    k = keys.view(np.float32)
    assert np.isfinite(k).all() and (k > 0).all() and (keys <= KEY_MAX).all()
    assert (k <= (37.0 / wt).astype(np.float32)).all()
    # a fixed-order float64 sum of at most 2^20 + 4096 positive terms
    np.testing.assert_allclose(rb.select_state()["den"], wt.sum(dtype=np.float64), rtol=1e-12)


@pytest.mark.parametrize("cap,n", [(c, n) for c, n in RINGS if c >= 5000],
                         ids=[i for i, (c, n) in zip(RING_IDS, RINGS) if c >= 5000])
def test_sample_selects_its_own_keys(rings, cap, n):
    """The production path: two samples (the second after the first has consumed and cleared the
    histograms), different draws."""
    rb, o = rings(cap, n)
    B = min(4096, n // 2)
    _check_sample(rb, o, B)
    k0 = rb.keys().cpu().numpy()[:n]
    _check_sample(rb, o, B)
    assert not np.array_equal(k0, rb.keys().cpu().numpy()[:n])


def test_select_state_carried_between_samples(gpu):
    """A tie case, a distinct case, an ordinary sample, then ties again on one ring: a stale tie
    count, an uncleared histogram copy or a stale prefix would show in the next one."""
    rb, o = _fill(5000, 5000, seed=1)
    rng = np.random.default_rng(9)
    _check_select(rb, o, _tie_keys(rng, 5000, TIE_CAP, 400), 400 + 64)
    _check_select(rb, o, _distinct_keys(rng, 5000), 4096)
    _check_sample(rb, o, 4096)
    _check_select(rb, o, _tie_keys(rng, 5000, 65, 300, T=0x00FFFFFF), 300 + 2)
    _check_sample(rb, o, 1)
    # even rows one pattern below the odd rows' key: 2500 equal keys under the threshold, one tie taken
    _check_select(rb, o, np.where(np.arange(5000) % 2 == 0, 0x3F7FFFFF, 0x3F800000).astype(np.uint32), 2501)
    assert rb.tie_overflows() == 0
    rb.close()


def test_select_keys_rejects_wrong_length(rings):
    from f110_gymnasium_ros2_jazzy_amd._lib import F110Error
    rb, o = rings(300, 211)
    with pytest.raises(F110Error):
        rb.select_keys(torch.zeros(210, dtype=torch.int64), BETA, 5)
    with pytest.raises(F110Error):
        rb.select_keys(torch.zeros(211, dtype=torch.int64), BETA, 212)


@pytest.mark.parametrize("n,n_tie,n_below,need", [(5000, 200, 300, 128), (5000, 5000, 0, 128), (20000, 6000, 1000, 4500),
                                                  (BIG, 5000, 3000, 4097)])
def test_tie_break_beyond_caps(gpu, n, n_tie, n_below, need):
    """More than 64 ties to take, and more ties than the tie list holds (kTieCap): the selection
    is still the lowest-index ties merged in index order; a list overflow is counted, and the
    ordinary sample that follows is exact."""
    rb, o = _fill(n, n, seed=2)
    rng = np.random.default_rng(n_tie)
    keys = np.full(n, 0x3F800000, np.uint32) if n_tie == n else _tie_keys(rng, n, n_tie, n_below)
    assert rb.tie_overflows() == 0
    idx = _check_select(rb, o, keys, n_below + need)
    assert idx.min() >= 0 and idx.max() < n and (np.diff(idx) > 0).all()
    if n_tie == n:
        np.testing.assert_array_equal(idx, np.arange(need))
    assert rb.tie_overflows() == (1 if n_tie > TIE_CAP else 0)
    _check_sample(rb, o, 4096)
    assert rb.tie_overflows() == (1 if n_tie > TIE_CAP else 0)
    rb.close()


def test_sample_with_replacement(gpu):
    """Fewer rows than the batch (k_sample_replace): 50 samples of 4096 i.i.d. draws from 7 rows
    follow p_i (|c - np| / sqrt(np(1 - p)) < 5 per row, the buffer's default seed), weights are
    the oracle's for the drawn indices; then update_priorities with a repeated index keeps the
    last value (k_update's serial path after a with-replacement sample)."""
    from f110_gymnasium_ros2_jazzy_amd.replay import DeviceReplayBuffer
    from replay_oracle import PEROracle
    prio = np.array([0.05, 3.0, 0.7, 1.0, 9.0, 0.2, 2.5], np.float32)
    rb = DeviceReplayBuffer(buffer_size=64, batch_size=4096, obs_dim=D, act_dim=A, device=0)
    o = PEROracle(64, 4096, alpha=0.6)
    z = torch.zeros(7, D, device="cuda")
    rb.add(z, z[:, :A], z[:, 0], z, priority=torch.from_numpy(prio))
    for p in prio:
        o.add(float(p))
    n_samples, B = 50, 4096
    counts = np.zeros(7, np.int64)
    for _ in range(n_samples):
        idx, _, w = rb.sample(beta=BETA, gather=False)
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        assert idx.min() >= 0 and idx.max() < 7
        np.testing.assert_allclose(w, o.weights(idx, BETA), rtol=2e-6)
        counts += np.bincount(idx, minlength=7)
    p = o.sampling_probs()
    N = n_samples * B
    z_score = np.abs(counts - N * p) / np.sqrt(N * p * (1 - p))
    print("with-replacement counts", counts.tolist(), "z", np.round(z_score, 2).tolist())
    assert z_score.max() < 5.0, (counts, N * p)
    upd_idx = np.array([3, 5, 3, 1, 3], np.int64)
    upd_val = np.array([1.0, 2.0, 3.0, 0.5, 4.0], np.float32)
    rb.update_priorities(upd_idx, upd_val)
    o.update_priorities(upd_idx, upd_val)
    got = rb.priorities().cpu().numpy()[:7]
    assert got[3] == 4.0 and got[5] == 2.0 and got[1] == 0.5
    np.testing.assert_array_equal(got, o.prio[:7])
    rb.close()
    # the largest batch a buffer takes (the kernel's LDS is sized by it)
    rb = DeviceReplayBuffer(buffer_size=64, batch_size=MAX_BATCH, obs_dim=D, act_dim=A, device=0)
    rb.add(z, z[:, :A], z[:, 0], z, priority=torch.from_numpy(prio))
    o.prio[:7] = prio
    idx, _, w = rb.sample(beta=BETA, gather=False)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert idx.shape == (MAX_BATCH,) and idx.min() >= 0 and idx.max() < 7
    np.testing.assert_allclose(w, o.weights(idx, BETA), rtol=2e-6)
    rb.close()
