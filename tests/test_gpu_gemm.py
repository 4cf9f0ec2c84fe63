"""
``lk_gemm_f32`` (csrc/spd_blocked.hip) through the C ABI: every op form, (alpha, beta) in
{(1, 0), (-1, 1)}, shapes that cross every tile edge, k = 0, leading dimensions above the row
length, the three tile masks.

Bound, per element, against the float64 product of the float32 operands: the MFMA sums a cell as
a chain of k fused multiply-adds, error <= k u (|A| |B|) to first order with u = 2^-24; the test
allows 2 k u (|A| |B|).  With beta != 0 the cell is then fmaf(alpha, sum, beta c), one more
rounding of a value no larger than |beta c| + |A| |B|: + u (|beta c| + |A| |B|).  With beta = 0
and alpha = +-1 nothing is added.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]
SHAPES = [(130, 70, 258), (1, 1, 1), (257, 129, 2), (33, 65, 0), (128, 128, 16), (129, 256, 17)]
SENTINEL = np.float32(-12345.678)


def _form_id(form):
    return ("T" if form[0] else "N") + ("T" if form[1] else "N")


def _padded(host: np.ndarray, pad: int, gpu):
    "A device copy of ``host`` inside a wider matrix of sentinels: (whole tensor, ld)."
    import torch

    r, c = host.shape
    whole = torch.full((max(r, 1), c + pad), float(SENTINEL), dtype=torch.float32, device=gpu)
    whole[:r, :c] = torch.from_numpy(host).to(gpu)
    return whole, c + pad


def _run(gpu, ta, tb, a, b, c0, alpha, beta, mask=0, pads=(3, 5, 7)):
    "One call on padded copies; returns C's whole padded buffer as a host array [m x ldc]."
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    lib = _native.require_gpu()
    m, n = c0.shape
    k = a.shape[0] if ta else a.shape[1]
    da, lda = _padded(a, pads[0], gpu)
    db, ldb = _padded(b, pads[1], gpu)
    dc, ldc = _padded(c0, pads[2], gpu)
    _native.check(lib.lk_gemm_f32(ta, tb, m, n, k, alpha, D._ptr(da), lda, D._ptr(db), ldb, beta,
                                  D._ptr(dc), ldc, mask, D._stream()), "lk_gemm_f32")
    torch.cuda.synchronize()
    return dc.cpu().numpy()[:m]


def _operands(rng, ta, tb, m, n, k):
    a = rng.standard_normal((k, m) if ta else (m, k)).astype(np.float32)
    b = rng.standard_normal((n, k) if tb else (k, n)).astype(np.float32)
    c0 = rng.standard_normal((m, n)).astype(np.float32)
    return a, b, c0


def _check(got, a, b, c0, ta, tb, alpha, beta, k):
    opa = (a.T if ta else a).astype(np.float64)
    opb = (b.T if tb else b).astype(np.float64)
    want = alpha * (opa @ opb) + (beta * c0.astype(np.float64) if beta else 0.0)
    mag = np.abs(opa) @ np.abs(opb)
    tol = 2 * k * U * mag
    if beta:
        tol = tol + U * (np.abs(beta * c0.astype(np.float64)) + mag)
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.max(err - tol)) if err.size else 0.0
    assert np.all(err <= tol), (worst, float(err.max()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_gemm_forms_bound_bits_and_padding(gpu, rng, form, shape):
    ta, tb = form
    m, n, k = shape
    a, b, c0 = _operands(rng, ta, tb, m, n, k)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
        start = c0 if beta else np.full_like(c0, np.nan)  # beta = 0: C is never read
        out = _run(gpu, ta, tb, a, b, start, alpha, beta)
        _check(out[:, :n], a, b, c0, ta, tb, alpha, beta, k)
        assert np.all(out[:, n:] == SENTINEL)  # the padding of C's rows is left alone
        again = _run(gpu, ta, tb, a, b, start, alpha, beta)
        assert np.array_equal(out.view(np.uint32), again.view(np.uint32))  # same bits


def test_gemm_tight_leading_dimensions(gpu, rng):
    "ld = the row length exactly (odd: rows 4-byte aligned only)."
    a, b, c0 = _operands(rng, 0, 1, 131, 67, 45)
    out = _run(gpu, 0, 1, a, b, c0, -1.0, 1.0, pads=(0, 0, 0))
    _check(out, a, b, c0, 0, 1, -1.0, 1.0, 45)


def test_gemm_offsets_past_2_31(gpu, rng):
    """Leading dimensions of 2^24 + 3 elements: the last rows of A and of C lie more than 2^31
    elements from their origins (the inverse of a 62 423-item Gramian addresses 3.9e9)."""
    import torch

    from lkpy_amd import _device as D

    m, n, k, ld = 130, 70, 40, (1 << 24) + 3
    assert (m - 1) * ld > 1 << 31
    a, b, c0 = _operands(rng, 0, 1, m, n, k)
    da = torch.empty((m, ld), dtype=torch.float32, device=gpu)  # (8.7 GB each, never filled)
    dc = torch.empty((m, ld), dtype=torch.float32, device=gpu)
    da[:, :k] = torch.from_numpy(a).to(gpu)
    dc[:, :n] = torch.from_numpy(c0).to(gpu)
    dc[:, n:n + 4] = float(SENTINEL)
    db = torch.from_numpy(b).to(gpu)
    D.gemm_f32(da[:, :k], db, dc[:, :n], trans_b=True, alpha=-1.0, beta=1.0)
    _check(dc[:, :n].cpu().numpy(), a, b, c0, 0, 1, -1.0, 1.0, k)
    assert bool((dc[:, n:n + 4] == float(SENTINEL)).all())
    # ... and as the transposed operand: A stored [k x m] with k = 130 rows of that pitch
    at = torch.empty((m, ld), dtype=torch.float32, device=gpu)
    at[:, :n] = torch.from_numpy(c0).to(gpu)  # op(A) = c0^T: [n x m], summed over the 130 rows
    out = torch.zeros((n, k), dtype=torch.float32, device=gpu)
    D.gemm_f32(at[:, :n], torch.from_numpy(a).to(gpu), out, trans_a=True)
    _check(out.cpu().numpy(), c0, a, np.zeros((n, k), np.float32), 1, 0, 1.0, 0.0, m)


def _tile_of(idx, tile):
    return np.asarray(idx) // tile


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_gemm_tile_masks(gpu, rng, form):
    """
    LOWER leaves the tiles above the diagonal untouched (sentinel); K_FROM_COL / K_FROM_ROW never
    read the part of the triangular operand they skip (it is NaN here) and give the product with
    that part zero.  Three tiles each way, ragged.
    """
    from lkpy_amd import _device as D
    from lkpy_amd import _native as N

    ta, tb = form
    t = D.gemm_tile()
    assert t == 128
    m = n = k = 2 * t + 37
    a, b, c0 = _operands(rng, ta, tb, m, n, k)
    ti = _tile_of(np.arange(m), t)
    upper_tiles = ti[:, None] < ti[None, :]  # cells of C in a tile above the diagonal
    # op(B)[kk][j] skipped where kk < first column of j's tile; op(A)[i][kk] where kk < first row
    skip_b = np.arange(k)[:, None] < (ti * t)[None, :]   # [k x n]
    skip_a = np.arange(k)[None, :] < (ti * t)[:, None]   # [m x k]

    def poisoned(x, skip, trans, value):
        y = x.copy()
        (y.T if trans else y)[skip] = value
        return y

    for mask, use_a, use_b in ((N.GEMM_LOWER, False, False), (N.GEMM_K_FROM_COL, False, True),
                               (N.GEMM_K_FROM_ROW, True, False),
                               (N.GEMM_LOWER | N.GEMM_K_FROM_ROW, True, False),
                               (N.GEMM_LOWER | N.GEMM_K_FROM_COL | N.GEMM_K_FROM_ROW, True, True)):
        lower = bool(mask & N.GEMM_LOWER)
        a_nan = poisoned(a, skip_a, ta, np.nan) if use_a else a
        b_nan = poisoned(b, skip_b, tb, np.nan) if use_b else b
        a_zero = poisoned(a, skip_a, ta, 0.0) if use_a else a
        b_zero = poisoned(b, skip_b, tb, 0.0) if use_b else b
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
            start = c0.copy()
            if lower:
                start[upper_tiles] = SENTINEL
            out = _run(gpu, ta, tb, a_nan, b_nan, start, alpha, beta, mask=mask)[:, :n]
            if lower:
                assert np.all(out[upper_tiles] == SENTINEL)  # masked-out tiles: untouched
            live = ~upper_tiles if lower else np.ones_like(upper_tiles)
            opa = (a_zero.T if ta else a_zero).astype(np.float64)
            opb = (b_zero.T if tb else b_zero).astype(np.float64)
            want = alpha * (opa @ opb) + beta * c0.astype(np.float64)
            mag = np.abs(opa) @ np.abs(opb)
            tol = 2 * k * U * mag + (U * (np.abs(beta * c0) + mag) if beta else 0.0)
            err = np.abs(out.astype(np.float64) - want)
            assert np.all(err[live] <= tol[live]), (mask, float(np.nanmax(err[live])))


def test_gemm_rejects_bad_arguments(gpu):
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    lib = _native.require_gpu()
    x = torch.zeros((4, 4), dtype=torch.float32, device=gpu)
    p, s = D._ptr(x), D._stream()
    assert lib.lk_gemm_f32(0, 0, 4, 4, 4, 1.0, p, 3, p, 4, 0.0, p, 4, 0, s) == _native.LK_E_INVALID
    assert lib.lk_gemm_f32(0, 0, 4, 4, 4, 1.0, p, 4, p, 4, 0.0, p, 4, 8, s) == _native.LK_E_INVALID
    assert lib.lk_gemm_f32(0, 0, -1, 4, 4, 1.0, p, 4, p, 4, 0.0, p, 4, 0, s) == _native.LK_E_INVALID
