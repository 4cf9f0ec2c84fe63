"""GPU parity, kernel level: the ragged candidate kernels of csrc/candidates.hip --
``lk_score_candidates`` (bit-equal to ``lk_score_dense`` and to the oracle's chain at every width
class), ``lk_panel_take_ragged`` and ``lk_ragged_topn`` (against ``tests/candidates_restatement``).
Everything is deterministic with a fixed order, so every comparison is bit equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import candidates_restatement as R

pytestmark = pytest.mark.gpu

N_ITEMS, N_USERS = 300, 40
WIDTHS = [1, 3, 4, 5, 63, 64, 66, 67, 128, 130, 1024]


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(R.bits(got)[~nan], R.bits(want)[~nan])


def _ptr(lens):
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr


# segment lengths: leading empty, the wave seam (63, 64, 65), consecutive empties in the middle,
# short ones, trailing empties
LAYOUT = [0, 63, 64, 65, 0, 0, 5, 1, 130, 0, 0]


@functools.lru_cache(maxsize=None)
def _layout(seed=7):
    "(ptr, items, user rows) of the mixed layout: invalid items and user rows sprinkled in"
    rng = np.random.default_rng(seed)
    ptr = _ptr(LAYOUT)
    items = rng.integers(0, N_ITEMS, int(ptr[-1])).astype(np.int32)
    items[rng.random(len(items)) < 0.05] = -1
    items[rng.random(len(items)) < 0.05] = N_ITEMS
    items[int(ptr[1])] = -1                  # first target of the batch
    items[int(ptr[-1]) - 1] = N_ITEMS        # the last one
    rows = rng.integers(0, N_USERS, len(LAYOUT)).astype(np.int32)
    rows[6], rows[7] = -1, N_USERS           # whole queries that cannot be scored
    rows[1], rows[8] = 0, N_USERS - 1
    return ptr, items, rows


@functools.lru_cache(maxsize=None)
def _operands(k):
    rng = np.random.default_rng(100 + k)
    return (rng.standard_normal((N_USERS, k)).astype(np.float32),
            rng.standard_normal((N_ITEMS, k)).astype(np.float32))


def _score(D, gpu, k, users, items_mat, rows, ptr, items):
    d_u, d_q = D.to_device_padded(users, gpu), D.to_device_padded(items_mat, gpu)
    got = D.score_candidates(d_u, d_q, k, _dev(rows, gpu), _dev(ptr, gpu), _dev(items, gpu), ptr)
    return got, d_u, d_q


@pytest.mark.parametrize("k", WIDTHS)
def test_score_candidates_is_the_dense_chain(gpu, oracle, k):
    from lkpy_amd import _device as D

    users, items_mat = _operands(k)
    ptr, items, rows = _layout()
    assert ptr[1] == 0 and ptr[-1] == ptr[-3] and (np.diff(ptr)[4:6] == 0).all()
    assert {63, 64, 65} <= set(np.diff(ptr).tolist())
    assert (items == -1).any() and (items == N_ITEMS).any()
    assert (rows == -1).any() and (rows == N_USERS).any()
    got, d_u, d_q = _score(D, gpu, k, users, items_mat, rows, ptr, items)
    got = _host(got)

    # the dense panel of the same operands, gathered
    panel = _host(D.score_dense(d_u, d_q, k))
    want = np.full(len(items), np.nan, np.float32)
    for q in range(len(rows)):
        for t in range(int(ptr[q]), int(ptr[q + 1])):
            if 0 <= rows[q] < N_USERS and 0 <= items[t] < N_ITEMS:
                want[t] = panel[rows[q], items[t]]
    bad_item = (items < 0) | (items >= N_ITEMS)
    bad_row = np.repeat((rows < 0) | (rows >= N_USERS), np.diff(ptr))
    assert np.array_equal(np.isnan(got), bad_item | bad_row)
    assert _same_bits(got, want)
    # ... and the oracle's restatement of the chain
    assert _same_bits(got, R.score_candidates_ref(oracle, users, items_mat, rows, ptr, items))

    # two runs: identical bits
    again = _host(_score(D, gpu, k, users, items_mat, rows, ptr, items)[0])
    assert np.array_equal(R.bits(got), R.bits(again))


@pytest.mark.parametrize("k", WIDTHS)
def test_score_candidates_one_long_segment(gpu, oracle, k):
    "5 000 targets of one query: a list split over many waves and workgroups"
    from lkpy_amd import _device as D

    users, items_mat = _operands(k)
    rng = np.random.default_rng(k)
    ptr = np.array([0, 5000], np.int64)
    items = rng.integers(0, N_ITEMS, 5000).astype(np.int32)
    items[[0, 4999]] = [N_ITEMS, -1]
    rows = np.array([17], np.int32)
    got = _host(_score(D, gpu, k, users, items_mat, rows, ptr, items)[0])
    want = R.score_candidates_ref(oracle, users, items_mat, rows, ptr, items)
    assert np.isnan(want[[0, 4999]]).all() and np.isnan(want).sum() == 2
    assert _same_bits(got, want)


def test_score_candidates_nothing_to_score(gpu):
    "total = 0 returns before the pointer checks (nothing is launched); bad offsets never launch"
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    lib = _native.require_gpu()
    null = ctypes.c_void_p(0)
    rc = lib.lk_score_candidates(null, 4, 0, null, 4, 0, 3, null, 5, null, null, 0, null, null)
    assert rc == 0
    users, items_mat = _operands(4)
    ptr = np.zeros(4, np.int64)
    got = _score(D, gpu, 4, users, items_mat, np.zeros(3, np.int32), ptr, np.zeros(0, np.int32))[0]
    assert got.shape == (0,)
    d_u, d_q = D.to_device_padded(users, gpu), D.to_device_padded(items_mat, gpu)
    items = np.zeros(6, np.int32)
    for bad in ([0, 4, 2, 6], [1, 2, 4, 6], [0, 2, 4, 5], [0, 2, 6]):
        bad = np.asarray(bad, np.int64)
        d_ptr = _dev(np.array([0, 2, 4, 6], np.int64), gpu)
        with pytest.raises(ValueError):
            D.score_candidates(d_u, d_q, 4, _dev(np.zeros(3, np.int32), gpu), d_ptr,
                               _dev(items, gpu), bad)


def test_panel_take_ragged(gpu, rng):
    from lkpy_amd import _device as D

    ptr = _ptr([0, 63, 64, 65, 0, 0, 5000 - 192])
    n_q, ld = len(ptr) - 1, N_ITEMS + 4
    assert n_q == 7 and ld > N_ITEMS
    panel = rng.standard_normal((n_q, ld)).astype(np.float32)
    panel[:, N_ITEMS:] = 12345.0  # the pad columns: never to be read
    panel[1, 5] = -0.0
    panel[2, 6] = np.nan
    items = rng.integers(0, N_ITEMS, int(ptr[-1])).astype(np.int32)
    items[rng.random(len(items)) < 0.05] = -1
    items[rng.random(len(items)) < 0.05] = N_ITEMS
    items[rng.random(len(items)) < 0.02] = N_ITEMS + 3
    items[0], items[1], items[int(ptr[2])] = N_ITEMS, 5, 6
    want = R.take_ragged_ref(panel, N_ITEMS, ptr, items)
    assert not (want == 12345.0).any() and np.signbit(want[1]) and want[1] == 0
    got = D.panel_take_ragged(_dev(panel, gpu), N_ITEMS, _dev(ptr, gpu), _dev(items, gpu), ptr)
    assert _same_bits(_host(got), want)
    empty = D.panel_take_ragged(_dev(panel, gpu), N_ITEMS, _dev(np.zeros(n_q + 1, np.int64), gpu),
                                _dev(np.zeros(0, np.int32), gpu), np.zeros(n_q + 1, np.int64))
    assert empty.shape == (0,)


# ---- lk_ragged_topn ------------------------------------------------------------------------------
NS = [1, 10, 64, 100, 5000, -1]
SPECIAL = np.array([-np.inf, np.inf, -0.0, 0.0, 0.0, -0.0, 1.5, 1.5, -2.25, np.nan], np.float32)


@functools.lru_cache(maxsize=None)
def _topn_case(wave_max, block_max):
    """
    One batch for every ``n``: random segments of every length the issue names (0, 1, n-1, n, n+1,
    one below / at / above each class boundary, 10 000) whose scores mix normals with NaN, +-inf,
    +-0.0 and repeated values, items drawn from a small range (repeats) with -1 sprinkled in; then
    the hand-made segments.
    """
    rng = np.random.default_rng(2024)
    lens = {0, 1, 2, 10000}
    for n in NS:
        if n > 0:
            lens |= {n - 1, n, n + 1}
    for b in (wave_max, block_max):
        lens |= {b - 1, b, b + 1}
    lens = sorted(lens)
    segs = []
    for ln in lens:
        sc = rng.standard_normal(ln).astype(np.float32)
        pick = rng.random(ln) < 0.3
        sc[pick] = rng.choice(SPECIAL, int(pick.sum()))
        it = rng.integers(0, 50, ln).astype(np.int32)
        it[rng.random(ln) < 0.05] = -1
        segs.append((it, sc))
    named = {}

    def add(name, it, sc):
        named[name] = len(segs)
        segs.append((np.asarray(it, np.int32), np.asarray(sc, np.float32)))

    for cls, ln in (("wave", 40), ("block", 200), ("sort", block_max + 500)):
        add(f"all_nan_{cls}", np.arange(ln), np.full(ln, np.nan))
        add(f"constant_{cls}", np.arange(ln)[::-1], np.full(ln, 0.75))
        z = np.where(np.arange(ln) % 2 == 0, -0.0, 0.0).astype(np.float32)
        z[ln // 2] = 1.0
        add(f"zeros_{cls}", np.arange(ln), z)
    add("zero_pair", [7, 8], [-0.0, 0.0])
    add("infs", [1, 2, 3, 4], [-np.inf, 5.0, np.inf, -np.inf])
    add("duplicate", [9, 9, 3], [1.0, 2.0, 1.0])
    add("negative_item", [4, -1, 6, -7], [1.0, 9.0, 2.0, 8.0])
    add("trailing_empty", [], [])
    ptr = _ptr([len(s[0]) for s in segs])
    items = np.concatenate([s[0] for s in segs]).astype(np.int32)
    scores = np.concatenate([s[1] for s in segs]).astype(np.float32)
    return lens, named, ptr, items, scores


@pytest.mark.parametrize("n", NS)
def test_ragged_topn(gpu, n):
    from lkpy_amd import _device as D

    wave_max, block_max = D.ragged_topn_classes()
    assert 1 < wave_max < block_max < 10000
    lens, named, ptr, items, scores = _topn_case(wave_max, block_max)
    for want_len in (0, 1, wave_max - 1, wave_max, wave_max + 1, block_max - 1, block_max,
                     block_max + 1, 10000) + ((n - 1, n, n + 1) if n > 0 else ()):
        assert want_len in lens
    want_i, want_s = R.ragged_topn_ref(ptr, items, scores, n)
    width = 10000 if n < 0 else n
    assert want_i.shape == (len(ptr) - 1, width)

    # the restatement shows the properties the kernel is held to
    for cls in ("wave", "block", "sort"):
        q = named[f"all_nan_{cls}"]
        assert (want_i[q] == -1).all() and np.isnan(want_s[q]).all()
        q = named[f"constant_{cls}"]  # the order is the positions: items were laid out descending
        ln = int(ptr[q + 1] - ptr[q])
        m = min(ln, width)
        assert np.array_equal(want_i[q, :m], np.arange(ln)[::-1][:m])
    if width >= 2:
        q = named["zero_pair"]
        assert want_i[q, :2].tolist() == [7, 8]
        assert R.bits(want_s[q, :2]).tolist() == [0x80000000, 0]
        assert want_i[named["duplicate"], :2].tolist() == [9, 9]
        assert want_i[named["infs"], :2].tolist() == [3, 2]
        assert want_i[named["negative_item"], :2].tolist() == [6, 4]
    if width >= 3:
        assert want_i[named["negative_item"], 2] == -1  # two entries dropped: padding follows
        assert np.isnan(want_s[named["negative_item"], 2])

    got_i, got_s = D.ragged_topn(_dev(ptr, gpu), _dev(items, gpu), _dev(scores, gpu), n, ptr)
    got_i, got_s = _host(got_i), _host(got_s)
    assert got_i.shape == want_i.shape and got_s.shape == want_s.shape
    for q in range(len(ptr) - 1):
        assert np.array_equal(got_i[q], want_i[q]), f"items of segment {q} (length {ptr[q + 1] - ptr[q]})"
        assert _same_bits(got_s[q], want_s[q]), f"scores of segment {q}"


def test_ragged_topn_short_batches(gpu, rng):
    "batches whose longest segment stays inside one class: the later kernels are not launched"
    from lkpy_amd import _device as D

    wave_max, block_max = D.ragged_topn_classes()
    for top in (wave_max, block_max):
        lens = [0, top, 3, top - 1, 0]
        ptr = _ptr(lens)
        scores = rng.standard_normal(int(ptr[-1])).astype(np.float32)
        scores[rng.random(len(scores)) < 0.2] = np.nan
        items = rng.integers(0, 9, len(scores)).astype(np.int32)
        for n in (5, -1):
            want_i, want_s = R.ragged_topn_ref(ptr, items, scores, n)
            got_i, got_s = D.ragged_topn(_dev(ptr, gpu), _dev(items, gpu), _dev(scores, gpu), n, ptr)
            assert np.array_equal(_host(got_i), want_i) and _same_bits(_host(got_s), want_s)
    # no queries, and no width
    none = D.ragged_topn(_dev(np.zeros(1, np.int64), gpu), _dev(np.zeros(0, np.int32), gpu),
                         _dev(np.zeros(0, np.float32), gpu), 10, np.zeros(1, np.int64))
    assert none[0].shape == (0, 10)
    zero = D.ragged_topn(_dev(ptr, gpu), _dev(items, gpu), _dev(scores, gpu), 0, ptr)
    assert zero[0].shape == (len(ptr) - 1, 0)
