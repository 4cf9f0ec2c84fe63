"""GPU parity: stable CSR transpose vs the oracle's restatement of transpose.rs -- BIT-EXACT."""
import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (300, 7), (7, 300), (5000, 70001)])
def test_transpose_bit_exact(gpu, oracle, rng, shape, is64):
    from lkpy_amd import _device as D

    n_rows, n_cols = shape
    m = sps.random(n_rows, n_cols, density=min(0.3, 2000.0 / (n_rows * n_cols) * 50),
                   format="csr", dtype=np.float32, random_state=int(rng.integers(1 << 30)))
    m.sort_indices()
    m.data = rng.standard_normal(m.nnz).astype(np.float32)
    dt = np.int64 if is64 else np.int32
    csr = D.DeviceCSR.from_arrays(m.indptr.astype(dt), m.indices, m.data, m.shape, gpu)
    t = D.csr_transpose(csr)
    ptr, idx, perm = oracle.transpose_csr(m.indptr.astype(dt), m.indices, n_cols)
    assert t.shape == (n_cols, n_rows)
    assert t.indptr.cpu().numpy().dtype == dt
    assert np.array_equal(t.indptr.cpu().numpy(), ptr)
    assert np.array_equal(t.indices.cpu().numpy(), idx)
    assert np.array_equal(t.perm.cpu().numpy(), perm)
    assert np.array_equal(t.values.cpu().numpy().view(np.uint32), m.data[perm].view(np.uint32))
    # transposing twice is the identity (columns of a row were sorted)
    tt = D.csr_transpose(t)
    assert np.array_equal(tt.indptr.cpu().numpy(), m.indptr.astype(dt))
    assert np.array_equal(tt.indices.cpu().numpy(), m.indices)
    assert np.array_equal(tt.values.cpu().numpy(), m.data)


def test_transpose_empty_and_structure_only(gpu, oracle):
    from lkpy_amd import _device as D
    from lkpy_amd.data import SparseRowArray

    e = sps.csr_array((4, 6), dtype=np.float32)
    t = D.csr_transpose(D.DeviceCSR.from_scipy(e, gpu))
    assert np.array_equal(t.indptr.cpu().numpy(), np.zeros(7, e.indptr.dtype)) and t.nnz == 0
    # the host data class goes through the same kernel (matrix.py:512-530)
    m = sps.random(40, 25, density=0.2, format="csr", dtype=np.float32, random_state=1)
    sra = SparseRowArray.from_scipy(m)
    tr = sra.transpose()
    want = sps.csr_array(m.T)
    want.sort_indices()
    assert tr.shape == (25, 40)
    assert np.array_equal(tr.offsets.to_numpy(), want.indptr)
    assert np.array_equal(tr.indices.to_numpy(), want.indices)
    assert np.array_equal(tr.values.to_numpy(), want.data)
    s_only = SparseRowArray.from_scipy(m, values=False).transpose()
    assert s_only.values is None and np.array_equal(s_only.indices.to_numpy(), want.indices)


@pytest.mark.parametrize("dtype,n", [("int32", 50_000_003), ("float32", 16_777_216 + 5), ("int64", 1000)])
def test_to_host_staged_download(gpu, dtype, n):
    "D.to_host: the pinned-ring / thread-team download returns exactly what .cpu() does"
    import torch

    from lkpy_amd import _device as D

    g = torch.Generator(device=gpu).manual_seed(3)
    if dtype == "float32":
        t = torch.randn(n, device=gpu, generator=g)
    else:
        t = torch.randint(-2**31 + 1, 2**31 - 1, (n,), device=gpu, generator=g,
                          dtype=getattr(torch, dtype))
    got = D.to_host(t, threads=6)
    assert got.dtype == np.dtype(dtype) and got.shape == (n,)
    assert np.array_equal(got, t.cpu().numpy())
    # a second transfer reuses the ring; a 2-D view keeps its shape
    t2 = t[: (n // 7) * 7].reshape(-1, 7)
    assert np.array_equal(D.to_host(t2), t2.cpu().numpy())


SORT_TILE = 4096  # keys per workgroup of the sort (radix_sort.h)


def _random_entries(rng, n_rows, n_cols, nnz):
    return np.sort(rng.integers(0, n_rows, nnz)), rng.integers(0, n_cols, nnz)


def _exact_entries(rng, n_cols, nnz):
    "exactly nnz distinct entries: rows of n_cols / 2 distinct random columns, the last one shorter"
    per = n_cols // 2
    n_rows = (nnz + per - 1) // per
    cols = np.argsort(rng.random((n_rows, n_cols)), axis=1)[:, :per].reshape(-1)[:nnz]
    return n_rows, np.repeat(np.arange(n_rows), per)[:nnz], cols


def _sort_case(name, rng):
    """(n_rows, n_cols, rows, cols, tiles, passes) of a named case: tiles and passes are what the
    case is there for (None: whatever the random draw leaves after de-duplication)"""
    if name == "tiles-256":
        n_rows, rows, cols = _exact_entries(rng, 2048, 256 * SORT_TILE)
        return n_rows, 2048, rows, cols, 256, 2
    if name == "tiles-257":  # one key in the last tile; the scan's second trip of 256 tiles
        n_rows, rows, cols = _exact_entries(rng, 2048, 256 * SORT_TILE + 1)
        return n_rows, 2048, rows, cols, 257, 2
    if name == "cols-256":  # 8 bits: one pass
        return (3000, 256, *_random_entries(rng, 3000, 256, 20000), None, 1)
    if name == "cols-257":  # 9 bits: two passes, the second one bit wide
        rows, cols = _random_entries(rng, 3000, 257, 20000)
        cols[::50] = 256  # (the only column with that bit set)
        return 3000, 257, rows, cols, None, 2
    if name == "cols-2^24+3":  # 25 bits: four passes; entries in the lowest and highest columns
        n_cols = 2 ** 24 + 3
        rows = np.sort(rng.integers(0, 50, 10000))
        cols = np.where(rng.random(10000) < 0.5, rng.integers(0, 300, 10000),
                        n_cols - 1 - rng.integers(0, 300, 10000))
        cols[:2] = [0, n_cols - 1]
        return 50, n_cols, rows, cols, None, 4
    assert name == "one-column"  # every key of a full tile shares every digit
    return 9000, 300, np.arange(9000), np.full(9000, 77), 3, 2


def _key_bits(n_cols):
    b = 1
    while b < 32 and (1 << b) < n_cols:
        b += 1
    return b


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("n_rows,n_cols,nnz", [(20000, 300, 3_000_000), (3000, 70001, 2_500_000),
                                                (10, 5, 37), (1, 100000, 4097), (4096, 4096, 4096),
                                                *[pytest.param(name, 0, 0, id=name) for name in
                                                  ("tiles-256", "tiles-257", "cols-256", "cols-257",
                                                   "cols-2^24+3", "one-column")]])
def test_transpose_hand_written_sort_sizes(gpu, oracle, rng, n_rows, n_cols, nnz, is64):
    """Round 6: the transpose's stable radix sort is this repository's own (csrc/radix_sort.h: 8-bit
    digits, 4096-key tiles; rounds 1-5 called rocPRIM).  Sizes that end inside a tile, span
    hundreds of tiles, take one / two / three / four digit passes; exactly 256 and 257 tiles; a
    last digit one bit wide; a tile of one single key value; heavy duplicate columns (stability is
    what keeps an output row's entries in source-row order); 32- and 64-bit offsets (``<uint32,
    uint32>`` and ``<uint32, uint64>`` pairs): offsets, indices and the permutation equal to the
    oracle's counting-sort transpose, entry for entry."""
    from lkpy_amd import _device as D

    tiles = passes = None
    if isinstance(n_rows, str):
        name = n_rows
        n_rows, n_cols, rows, cols, tiles, passes = _sort_case(name, rng)
        nnz = len(rows)
    else:
        rows, cols = _random_entries(rng, n_rows, n_cols, nnz)
    m = sps.csr_array((np.ones(nnz, np.float32), (rows, cols)), shape=(n_rows, n_cols))
    m.sum_duplicates()
    m.sort_indices()
    m.data = rng.standard_normal(m.nnz).astype(np.float32)
    # the edges a named case claims are there after de-duplication
    if tiles is not None:
        assert m.nnz == nnz and (m.nnz + SORT_TILE - 1) // SORT_TILE == tiles
    if passes is not None:
        assert (_key_bits(n_cols) + 7) // 8 == passes
        assert m.indices.min() == 0 or name == "one-column"
        if name == "cols-257":
            assert _key_bits(n_cols) == 9 and (m.indices == 256).sum() > 100
        if name == "cols-2^24+3":
            assert _key_bits(n_cols) == 25 and m.indices.max() == n_cols - 1
            assert (m.indices < 300).sum() > 4000 and (m.indices >= n_cols - 300).sum() > 4000
        if name == "one-column":
            assert m.nnz > 2 * SORT_TILE and len(np.unique(m.indices)) == 1
    dt = np.int64 if is64 else np.int32
    csr = D.DeviceCSR.from_arrays(m.indptr.astype(dt), m.indices, m.data, m.shape, gpu)
    assert csr.is64 == is64
    t = D.csr_transpose(csr)
    ptr, idx, perm = oracle.transpose_csr(m.indptr.astype(dt), m.indices, n_cols)
    assert t.indptr.cpu().numpy().dtype == dt and t.perm.cpu().numpy().dtype == dt
    assert np.array_equal(t.indptr.cpu().numpy(), ptr)
    assert np.array_equal(t.indices.cpu().numpy(), idx)
    assert np.array_equal(t.perm.cpu().numpy(), perm)
