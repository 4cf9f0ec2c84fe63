"""GPU parity, kernel level: the batch scoring kernels (``lk_ease_score_batch``,
``lk_slim_score_batch``, ``lk_take_scores``, ``lk_csr_rows_dot``, ``lk_score_dense``) and the
large-result downloads (``lk_download``, ``lk_download_i32_narrow``) at their own edges.

Every kernel here is deterministic with a fixed summation order, so every comparison is bit
equality against ``tests/batch_restatement.py`` (NaN where NaN, the same bits elsewhere).  Each test
first asserts, on its own inputs, that the edges it claims are present."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import batch_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF  # a finite float32 bit pattern no score takes


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _sentinel(shape, gpu):
    return _dev(np.full(shape, SENTINEL, np.uint32).view(np.float32), gpu)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _ptr_of(hist):
    ptr = np.zeros(len(hist) + 1, np.int64)
    np.cumsum([len(h) for h in hist], out=ptr[1:])
    items = np.concatenate([np.asarray(h, np.int32) for h in hist]).astype(np.int32)
    return ptr, items


def _abi():
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    return _native.require_gpu(), D, _native.check


# ---- 1. lk_ease_score_batch ---------------------------------------------------------------------


@pytest.mark.parametrize("n_items", [1, 255, 256, 257, 1000])
def test_ease_score_batch_strips_and_padding(gpu, rng, n_items):
    lib, D, check = _abi()
    n = n_items
    w = R.magnitudes(rng, (n, n))
    long = rng.permutation(n)[: min(300, n)]
    hist = [[], [n - 1], [n // 2, n // 2], [-1, n, n + 5], long]
    while len(hist) < 12:
        h = rng.integers(0, n, int(rng.integers(1, 30)))
        h[rng.random(len(h)) < 0.15] = rng.choice([-1, n, n + 5])
        hist.append(h)
    ptr, items = _ptr_of(hist)
    B = len(hist)
    assert B == 12 and ptr[1] == 0 and ptr[2] - ptr[1] == 1
    assert hist[2][0] == hist[2][1] and len(hist[4]) == min(300, n)
    assert all(it < 0 or it >= n for it in hist[3])
    assert len(np.unique(long)) == len(long) and (n < 3 or np.any(np.diff(long) < 0))
    want = R.ease_score(w, ptr, items)
    assert not want[0].any() and not want[3].any() and not np.isnan(want).any()
    assert np.array_equal(want[2], w[n // 2] + w[n // 2])  # counted twice at this level

    got = D.ease_score_batch(_dev(ptr, gpu), _dev(items, gpu), _dev(w, gpu))
    assert got.shape == (B, n) and np.array_equal(_bits(got), want.view(np.uint32))

    # padded leading dimensions: NaN in the weights' pad columns, a sentinel under the output
    ld_w, ld_out = n + 3, n + 5
    wp = np.full((n, ld_w), np.nan, np.float32)
    wp[:, :n] = w
    d_ptr, d_items, d_w = _dev(ptr, gpu), _dev(items, gpu), _dev(wp, gpu)
    out = _sentinel((B, ld_out), gpu)
    check(lib.lk_ease_score_batch(D._ptr(d_ptr), D._ptr(d_items), B, D._ptr(d_w), n, ld_w,
                                  D._ptr(out), ld_out, D._stream()), "lk_ease_score_batch")
    got = _bits(out)
    assert np.all(got[:, n:] == SENTINEL)
    assert not np.isnan(got[:, :n].view(np.float32)).any()
    assert np.array_equal(got[:, :n], want.view(np.uint32))


def test_ease_score_batch_query_seam(gpu, rng):
    "65 538 queries: the wrapper's second launch (grid.y holds 65 535) serves the last three."
    _lib, D, _check = _abi()
    B, n = 65538, 5
    lens = rng.integers(0, 4, B)
    lens[65534:] = [1, 0, 3, 2]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    items = rng.integers(-1, n + 1, int(ptr[-1])).astype(np.int32)
    items[ptr[65534]:] = [4, 0, 3, 0, 2, 1]  # known items behind the seam
    w = R.magnitudes(rng, (n, n))
    assert B > 65535 and (np.diff(ptr)[65534:] > 0).sum() == 3
    assert (lens == 0).any() and (items == -1).any() and (items == n).any()
    want = R.ease_score(w, ptr, items)
    assert all(want[q].any() for q in (65534, 65536, 65537)) and not want[65535].any()
    got = D.ease_score_batch(_dev(ptr, gpu), _dev(items, gpu), _dev(w, gpu))
    assert got.shape == (B, n) and np.array_equal(_bits(got), want.view(np.uint32))


# ---- 2. lk_slim_score_batch ---------------------------------------------------------------------

SLIM_N = 1000
SLIM_ROWS = {10: 0, 11: 1, 12: 255, 13: 256, 14: 257, 15: 700}  # weight row -> its length


@pytest.fixture(scope="module")
def slim_case():
    "Weights, queries and the restatement's panels for every mark: computed once, never changed."
    rng = np.random.default_rng(7)
    n = SLIM_N
    lens = rng.integers(2, 40, n)
    for r, m in SLIM_ROWS.items():
        lens[r] = m
    w_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=w_ptr[1:])
    w_idx = np.concatenate([np.sort(rng.choice(n, m, replace=False)) for m in lens])
    w = sps.csr_array((R.magnitudes(rng, len(w_idx)), w_idx.astype(np.int32), w_ptr), shape=(n, n))
    hist = [[], [-1, n, n + 5], [15, 15, 20], rng.permutation(n)[:300], [0, 999],
            [12, 13, 14, 15, 11, 10], [999, -1, 0, n, 15], []]
    while len(hist) < 40:
        h = rng.integers(0, n, int(rng.integers(1, 30)))
        h[rng.random(len(h)) < 0.1] = rng.choice([-1, n, n + 7])
        hist.append(h)
    hist[39] = [14, n, 3, 3, -1, 999]
    ptr, items = _ptr_of(hist)
    want = {mark: R.slim_score(w, ptr, items, mark) for mark in range(4)}
    for v in want.values():
        v.setflags(write=False)
    _slim_edges_present(w, hist, want)
    return w, hist, ptr, items, want


def _slim_edges_present(w, hist, want):
    "Every test of the shared case asserts its edges through the fixture."
    lens = np.diff(w.indptr)
    assert all(lens[r] == m for r, m in SLIM_ROWS.items()) and w.shape == (SLIM_N, SLIM_N)
    assert len(hist) == 40 and len(hist[0]) == 0 and len(hist[7]) == 0
    assert all(it < 0 or it >= SLIM_N for it in hist[1])
    assert hist[2][0] == hist[2][1] and len(hist[3]) == 300 and len(set(hist[3])) == 300
    assert 0 in hist[4] and 999 in hist[4]
    # history order: query 5's rows share targets, and adding them in reverse changes bits
    shared = set(w.indices[w.indptr[12]:w.indptr[13]]) & set(w.indices[w.indptr[13]:w.indptr[14]])
    assert len(shared) > 10
    rev = R.slim_score(w, *_ptr_of([hist[5][::-1]]), 0)[0]
    assert (rev.view(np.uint32) != want[0][5].view(np.uint32)).any()
    # the mark bits: struck items, an all-NaN empty row, an unknown-only row that stays zero
    assert np.isnan(want[1][4][[0, 999]]).all() and not np.isnan(want[1][0]).any()
    assert np.isnan(want[2][0]).all() and not np.isnan(want[2][1]).any() and not want[3][1].any()
    assert np.isnan(want[3][39][[14, 3, 999]]).all() and np.isnan(want[3][39]).sum() == 3
    assert not np.isnan(want[0]).any()
    assert any(len(hist[q]) == 0 for q in range(3, 17))  # an empty history inside a window


def _slim_weights_dev(w, gpu):
    from lkpy_amd import _device as D

    return D.DeviceCSR(_dev(w.indptr.astype(np.int64), gpu), _dev(w.indices.astype(np.int32), gpu),
                       _dev(w.data.astype(np.float32), gpu), w.shape, None)


@pytest.mark.parametrize("mark", [0, 1, 2, 3])
def test_slim_score_batch_marks_and_windows(gpu, slim_case, mark):
    _lib, D, _check = _abi()
    w, hist, ptr, items, want = slim_case
    d_w, d_ptr, d_items = _slim_weights_dev(w, gpu), _dev(ptr, gpu), _dev(items, gpu)
    for rows in (None, (3, 17), (39, 40), (5, 5)):
        lo, hi = rows if rows is not None else (0, len(hist))
        got = D.slim_score_batch(d_ptr, d_items, d_w, rows=rows, strike_history=bool(mark & 1),
                                 nan_empty=bool(mark & 2))
        assert tuple(got.shape) == (hi - lo, SLIM_N), rows
        assert R.same_bits(got.cpu().numpy(), want[mark][lo:hi]), (mark, rows)


def test_slim_score_batch_padded_output(gpu, slim_case):
    lib, D, check = _abi()
    w, hist, ptr, items, want = slim_case
    d_w, d_ptr, d_items = _slim_weights_dev(w, gpu), _dev(ptr, gpu), _dev(items, gpu)
    B, ld_out = len(hist), SLIM_N + 7
    out = _sentinel((B, ld_out), gpu)
    check(lib.lk_slim_score_batch(D._ptr(d_ptr), D._ptr(d_items), B, D._ptr(d_w.indptr),
                                  D._ptr(d_w.indices), D._ptr(d_w.values), SLIM_N, D._ptr(out),
                                  ld_out, 3, D._stream()), "lk_slim_score_batch")
    got = _bits(out)
    assert np.all(got[:, SLIM_N:] == SENTINEL)
    assert R.same_bits(got[:, :SLIM_N].view(np.float32), want[3])


# ---- 3. lk_take_scores --------------------------------------------------------------------------

TAKE_SPECIAL = {0: 0x7F800000, 1: 0xFF800000, 2: 0x80000000,  # +inf, -inf, -0.0
                3: 0x7FC00001, 4: 0xFFC12345, 5: 0x7F800001}  # NaNs with distinct payloads


@pytest.mark.parametrize("n", [1, 10, 257])
def test_take_scores_bits(gpu, rng, n):
    _lib, D, _check = _abi()
    rows, row_len = 37, 1000
    panel = rng.standard_normal((rows, row_len)).astype(np.float32)
    for c, pattern in TAKE_SPECIAL.items():
        panel.view(np.uint32)[:, c] = pattern
    planted = [-1, row_len, 2 ** 31 - 1, *TAKE_SPECIAL, row_len - 1]
    flat = rng.integers(0, row_len, rows * n).astype(np.int32)
    flat[: len(planted)] = planted
    tail = flat[len(planted)::13]
    tail[:] = np.resize(planted, len(tail))
    idx = flat.reshape(rows, n)
    assert (rows * n) % 256 != 0 and np.isfinite(panel[:, 6:]).all()
    assert all((idx == v).any() for v in planted)
    want = R.take_scores(panel, idx)
    ok = (idx >= 0) & (idx < row_len)
    assert ok.any() and (~ok).sum() >= 3
    assert all((want.view(np.uint32)[ok] == p).any() for p in TAKE_SPECIAL.values())
    got = D.take_scores(_dev(panel, gpu), _dev(idx, gpu))
    assert tuple(got.shape) == (rows, n)
    got = _bits(got)
    assert np.isnan(got.view(np.float32)[~ok]).all()
    # valid cells: the panel's exact bits, NaN payloads included
    assert np.array_equal(got[ok], want.view(np.uint32)[ok])
    assert R.same_bits(got.view(np.float32), want)


# ---- 4. lk_csr_rows_dot -------------------------------------------------------------------------

DOT_LENS = [0, 1, 63, 64, 65, 129, 200]
DOT_COLS = 300


def _dot_matrix(rng):
    ptr = np.zeros(len(DOT_LENS) + 1, np.int64)
    np.cumsum(DOT_LENS, out=ptr[1:])
    idx = np.concatenate([rng.permutation(DOT_COLS)[:m] for m in DOT_LENS]).astype(np.int32)
    csr = sps.csr_array((R.magnitudes(rng, len(idx)), idx, ptr), shape=(len(DOT_LENS), DOT_COLS))
    assert len(DOT_LENS) % 4 != 0 and list(np.diff(csr.indptr)) == DOT_LENS
    assert np.array_equal(csr.indices, idx)  # entry order is the chain's order: kept as drawn
    return csr


def _dot_dev(csr, is64, gpu):
    from lkpy_amd import _device as D

    d = D.DeviceCSR(_dev(csr.indptr.astype(np.int64 if is64 else np.int32), gpu),
                    _dev(csr.indices.astype(np.int32), gpu),
                    _dev(csr.data.astype(np.float32), gpu), csr.shape, None)
    assert d.is64 == is64
    return d


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_csr_rows_dot_bit_exact(gpu, oracle, rng, B, is64):
    _lib, D, _check = _abi()
    csr = _dot_matrix(rng)
    x = R.magnitudes(rng, (DOT_COLS, B))
    want = R.csr_rows_dot(csr, x, oracle)
    assert not want[:, 0].any() and np.all(want[:, 1:] != 0)
    got = D.csr_rows_dot(_dot_dev(csr, is64, gpu), _dev(x, gpu))
    assert tuple(got.shape) == (B, len(DOT_LENS))
    assert np.array_equal(_bits(got), want.view(np.uint32))


def test_csr_rows_dot_padded(gpu, oracle, rng):
    lib, D, check = _abi()
    csr = _dot_matrix(rng)
    B, n_rows = 65, len(DOT_LENS)
    ld_x, ld_out = B + 2, n_rows + 3
    x = R.magnitudes(rng, (DOT_COLS, B))
    xp = np.full((DOT_COLS, ld_x), np.nan, np.float32)
    xp[:, :B] = x
    want = R.csr_rows_dot(csr, x, oracle)
    d, d_x, out = _dot_dev(csr, True, gpu), _dev(xp, gpu), _sentinel((B, ld_out), gpu)
    check(lib.lk_csr_rows_dot(D._ptr(d.indptr), 1, D._ptr(d.indices), D._ptr(d.values), n_rows,
                              D._ptr(d_x), ld_x, B, D._ptr(out), ld_out, D._stream()),
          "lk_csr_rows_dot")
    got = _bits(out)
    assert np.all(got[:, n_rows:] == SENTINEL)
    assert not np.isnan(got[:, :n_rows].view(np.float32)).any()
    assert np.array_equal(got[:, :n_rows], want.view(np.uint32))


# ---- 5. lk_score_dense --------------------------------------------------------------------------


def _dense_case(rng, B, I, k):
    U, Q = R.magnitudes(rng, (B, k)), R.magnitudes(rng, (I, k))
    zero = np.arange(3, I, 61)  # a few all-zero item rows (unrated items), the last tile included
    Q[zero] = 0.0
    return U, Q, zero


@pytest.mark.parametrize("B,I,k", [(1, 1, 1), (1, 1000, 25), (63, 255, 16), (64, 256, 17),
                                   (65, 257, 100), (130, 1000, 300)])
def test_score_dense_bit_exact(gpu, oracle, rng, B, I, k):
    _lib, D, _check = _abi()
    U, Q, zero = _dense_case(rng, B, I, k)
    want = R.dense_scores(Q, U, oracle)
    assert I < 8 or (len(zero) >= 3 and not want[:, zero].any())
    assert np.count_nonzero(want) == B * (I - len(zero))
    got = D.score_dense(D.to_device_padded(U, gpu), D.to_device_padded(Q, gpu), k)
    assert tuple(got.shape) == (B, I)
    got = _bits(got)
    for b in range(B):
        assert np.array_equal(got[b], want[b].view(np.uint32)), b


def test_score_dense_padded_output(gpu, oracle, rng):
    lib, D, check = _abi()
    B, I, k = 65, 257, 100
    U, Q, _zero = _dense_case(rng, B, I, k)
    want = R.dense_scores(Q, U, oracle)
    d_u, d_q = D.to_device_padded(U, gpu), D.to_device_padded(Q, gpu)
    kp, ld_out = D.padded_dim(k), I + 9
    assert kp > k and tuple(d_u.shape) == (B, kp)
    out = _sentinel((B, ld_out), gpu)
    check(lib.lk_score_dense(D._ptr(d_u), kp, B, D._ptr(d_q), kp, I, k, D._ptr(out), ld_out,
                             D._stream()), "lk_score_dense")
    got = _bits(out)
    assert np.all(got[:, I:] == SENTINEL)
    assert np.array_equal(got[:, :I], want.view(np.uint32))


# ---- 6. downloads -------------------------------------------------------------------------------

DL_CHUNK = 8 << 20  # bytes per staging slot (misc.hip)
DL_SLOTS = 24


def _index_tensor(gpu, n, chunk_elems, bound=65536):
    """int32 [n] in [0, bound) with 0 and bound-1 planted at both ends and on both sides of every
    staging-chunk boundary; returns the tensor and the number of chunks it crosses in."""
    g = torch.Generator(device=gpu).manual_seed(11)
    t = torch.randint(0, bound, (n,), device=gpu, generator=g, dtype=torch.int32)
    edges = torch.arange(chunk_elems, n, chunk_elems, device=gpu)
    t[edges - 1] = bound - 1
    t[edges] = 0
    t[0], t[n - 1] = 0, bound - 1
    return t, (n + chunk_elems - 1) // chunk_elems


@pytest.mark.parametrize("n", [16_777_216, 16_777_221, 104_857_603])
def test_download_narrow(gpu, n):
    "uint16 across the link, int32 on the host: whole chunks, a 10-byte tail, slots re-used."
    _lib, D, _check = _abi()
    per = DL_CHUNK // 2
    t, chunks = _index_tensor(gpu, n, per)
    want = t.cpu().numpy()
    assert n * 4 >= 64 << 20 and n * 2 >= 4 * DL_CHUNK  # D.to_host stages it through the ring
    assert chunks == {16_777_216: 4, 16_777_221: 5, 104_857_603: 26}[n]
    assert (n * 2) % DL_CHUNK == {16_777_216: 0, 16_777_221: 10, 104_857_603: 6}[n]
    assert want[0] == 0 and want[-1] == 65535 and want[per - 1] == 65535 and want[per] == 0
    last = (chunks - 1) * per
    assert want[last - 1] == 65535 and (last == n or want[last] in (0, 65535))
    assert int(want.min()) == 0 and int(want.max()) == 65535
    for threads in (1, 6, 0):
        got = D.to_host(t, threads=threads, index_bound=65536)
        assert got.dtype == np.int32 and got.shape == (n,)
        assert np.array_equal(got, want), threads
    if chunks > DL_SLOTS:  # a 2-D tensor keeps its shape
        rows = n // 7
        t2, want2 = t[: rows * 7].reshape(rows, 7), want[: rows * 7].reshape(rows, 7)
        assert rows * 7 * 2 > DL_SLOTS * DL_CHUNK
        got = D.to_host(t2, threads=0, index_bound=65536)
        assert got.dtype == np.int32 and got.shape == (rows, 7) and np.array_equal(got, want2)


def test_download_narrow_not_taken(gpu, monkeypatch):
    "A bound above 65 536, or LK_DOWNLOAD_NARROW=0, is the plain path."
    _lib, D, _check = _abi()
    n = 16_777_221
    t, _chunks = _index_tensor(gpu, n, DL_CHUNK // 4, bound=65537)
    want = t.cpu().numpy()
    assert int(want.max()) == 65536 and want[-1] == 65536  # the narrow path would lose this
    got = D.to_host(t, threads=6, index_bound=65537)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    t, _chunks = _index_tensor(gpu, n, DL_CHUNK // 4)
    want = t.cpu().numpy()
    assert int(want.max()) == 65535
    monkeypatch.setenv("LK_DOWNLOAD_NARROW", "0")
    got = D.to_host(t, threads=6, index_bound=65536)
    assert got.dtype == np.int32 and got.shape == (n,) and np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 1001])
def test_download_narrow_small_branch(gpu, rng, n):
    "Below four chunks the ABI copies in one piece and widens on the host: only reachable directly."
    lib, D, check = _abi()
    src = rng.integers(0, 65536, n).astype(np.int32)
    src[0] = 65535
    src[-1] = 0 if n > 1 else 65535
    guard = -0x5A5A5A5B
    host = np.full(n + 1, guard, np.int32)
    d_src = _dev(src, gpu)
    tmp = torch.empty(n, dtype=torch.int16, device=gpu)
    assert n * 2 < 4 * DL_CHUNK and (src == 65535).any()
    check(lib.lk_download_i32_narrow(host.ctypes.data_as(ctypes.c_void_p), D._ptr(d_src), n,
                                     D._ptr(tmp), 0, D._stream()), "lk_download_i32_narrow")
    assert np.array_equal(host[:n], src) and host[n] == guard


def test_download_beyond_the_ring(gpu):
    "26 chunks through 24 slots: slots 0 and 1 are re-used; the ring stays usable afterwards."
    _lib, D, _check = _abi()
    n = 52_428_803
    assert (n * 4 + DL_CHUNK - 1) // DL_CHUNK == DL_SLOTS + 2 and (n * 4) % DL_CHUNK == 12
    g = torch.Generator(device=gpu).manual_seed(5)
    t = torch.randint(-2**31 + 1, 2**31 - 1, (n,), device=gpu, generator=g, dtype=torch.int32)
    want = t.cpu().numpy()
    got = D.to_host(t, threads=6)
    assert got.dtype == np.int32 and got.shape == (n,) and np.array_equal(got, want)
    # the same bits as float32: NaN payloads of every kind among them
    f = t.view(torch.float32)
    f[0], f[n - 1] = float("nan"), float("-inf")
    want = f.cpu().numpy().view(np.uint32)
    nan = (want & 0x7FFFFFFF) > 0x7F800000
    assert nan.sum() > 1000 and len(np.unique(want[nan][:4096])) > 1000
    got = D.to_host(f, threads=0)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got.view(np.uint32), want)
    del got, want, nan
    # a second, small staged transfer right after
    m = 16_777_221
    t2 = t[:m].contiguous()
    assert m * 4 >= 4 * DL_CHUNK and (m * 4) % DL_CHUNK == 20
    assert np.array_equal(D.to_host(t2, threads=6), t2.cpu().numpy())
