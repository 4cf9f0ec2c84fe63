"""
NumPy restatement of the CG solver's row solve (csrc/als_cg.hip), with the arithmetic type as a
parameter, and the test matrix whose row lengths sit on every seam of that kernel.  It calls
nothing of the package: the kernel (tests/test_gpu_als_cg.py) and the restatement's own float64
run (tests/test_als_cg_host.py, against ``np.linalg.solve``) are both held to it.

The operation, per CSR row with entries (j, v_j) and the other side's factor rows q_j:

    A = OtOr + sum_j v_j q_j q_j^T           (formed densely here; the kernel never forms it)
    y = sum_j (v_j + 1) q_j
    d = diag(OtOr) + sum_j v_j q_j^2,   dinv = 1 / d        (Jacobi preconditioner)
    x = x0 (warm start);  r = y - A x;  z = r * dinv;  p = z;  stop = tol^2 (y . y)
    while it < max_iter and r . r > stop:
        alpha = (r . z) / (p . A p);  x += alpha p;  r -= alpha A p;  z = r * dinv
        beta = (r . z)_new / (r . z);  p = z + beta p

An empty row is zeros after no iteration; ``max_iter = 0`` means k (``launch_cg``).  Every sum is
NumPy's own in the requested type: the restatement fixes the operation, not a summation order.

``variant`` perturbs the definition on purpose, for the host tests that prove the GPU bounds can
tell a wrong kernel from a right one (tests/test_als_cg_host.py): ``"shift"`` pairs each value with
the next entry of its row, ``"nojacobi"`` sets dinv = 1.
"""
import functools
import types

import numpy as np
import scipy.sparse as sps

N_COLS = 2100
REG = 0.1


def resident(kp: int) -> int:
    "RI: the entries one wave keeps in registers (4096 / KP)"
    return 4096 // kp


def tail_batch(kp: int) -> int:
    "TB: the tail entries a wave gathers per batch"
    return 16 if kp <= 128 else 8


def padded(k: int) -> int:
    "the CG kernel's padded widths (k > 32)"
    assert 32 < k <= 256
    return 64 if k <= 64 else (128 if k <= 128 else 256)


def seam_lengths(kp: int) -> list:
    ri, tb = resident(kp), tail_batch(kp)
    lens = {1, 2, 7, 8, 9,
            ri - 1, ri, ri + 1, ri + 8,
            2 * ri - 1, 2 * ri, 2 * ri + 1, 3 * ri + 1,
            4 * ri - 9, 4 * ri - 8, 4 * ri - 1, 4 * ri, 4 * ri + 1,
            4 * ri + tb - 1, 4 * ri + tb, 4 * ri + tb + 1, 4 * ri + 4 * tb, 4 * ri + 4 * tb + 1,
            4 * ri + 9 * tb + 3,
            2048, 2049}
    return sorted(lens)


def seam_matrix(kp: int, seed: int, k: int = None, negative: bool = False):
    """
    -> (csr float32 [rows x 2100], other float32 [2100 x k], this float32 [rows x k]).

    Every seam length twice and three empty rows, in a seeded shuffled order; sorted distinct
    columns; values uniform(0, 40) with about 10 % exactly 0 (``negative``: a further 10 % times
    -0.05); ``other`` = standard_normal * a shuffled geomspace(0.05, 0.2, k) per column; ``this`` =
    standard_normal * 0.1.  ``k`` defaults to ``kp``.
    """
    k = kp if k is None else k
    rng = np.random.default_rng(seed)
    lens = np.array(seam_lengths(kp) * 2 + [0, 0, 0], dtype=np.int64)
    rng.shuffle(lens)
    n_rows = len(lens)
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.empty(indptr[-1], np.int32)
    for r in range(n_rows):
        indices[indptr[r]:indptr[r + 1]] = np.sort(
            rng.choice(N_COLS, lens[r], replace=False)).astype(np.int32)
    values = rng.uniform(0.0, 40.0, indptr[-1]).astype(np.float32)
    u = rng.random(indptr[-1])
    values[u < 0.1] = 0.0
    if negative:
        values[(u >= 0.1) & (u < 0.2)] *= np.float32(-0.05)
    scale = np.geomspace(0.05, 0.2, k)
    rng.shuffle(scale)
    other = (rng.standard_normal((N_COLS, k)) * scale).astype(np.float32)
    this = (rng.standard_normal((n_rows, k)) * 0.1).astype(np.float32)
    mat = sps.csr_array((values, indices, indptr), shape=(n_rows, N_COLS))
    return mat, other, this


def otor32(other: np.ndarray, reg: float = REG) -> np.ndarray:
    "OtOr = other^T other + reg I, summed in float64 and rounded once to float32"
    o64 = np.asarray(other, np.float64)
    return (o64.T @ o64 + reg * np.eye(o64.shape[1])).astype(np.float32)


def row_system(q, v, otor, dtype=np.float64, variant=None):
    "-> (A, y, dinv) of one row in ``dtype``"
    q = np.asarray(q, dtype)
    v = np.asarray(v, dtype)
    otor = np.asarray(otor, dtype)
    if variant == "shift":
        v = np.roll(v, -1)
    A = otor + (q.T * v) @ q
    y = q.T @ (v + dtype(1.0))
    d = np.diagonal(otor) + (q * q).T @ v
    dinv = np.ones_like(d) if variant == "nojacobi" else dtype(1.0) / d
    assert A.dtype == dtype and y.dtype == dtype and dinv.dtype == dtype
    return A, y, dinv


def cg_row(q, v, otor, x0, tol, max_iter=0, dtype=np.float64, variant=None):
    """
    One row's solve as the kernel defines it -> (x, iterations, [r.r before every iteration and
    after the last]).  ``q``: the row's gathered factor rows [n x k], ``v``: its values [n].
    """
    k = np.asarray(otor).shape[0]
    if len(v) == 0:
        return np.zeros(k, dtype), 0, []
    if max_iter == 0:
        max_iter = k
    A, y, dinv = row_system(q, v, otor, dtype, variant)
    x = np.array(x0, dtype)
    r = y - A @ x
    z = r * dinv
    p = z.copy()
    rz = r @ z
    rr = r @ r
    stop = dtype(tol) * dtype(tol) * (y @ y)
    hist = [float(rr)]
    it = 0
    while it < max_iter and rr > stop:
        ap = A @ p
        alpha = rz / (p @ ap)
        x = x + alpha * p
        r = r - alpha * ap
        z = r * dinv
        rz_new = r @ z
        rr = r @ r
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        it += 1
        hist.append(float(rr))
    assert x.dtype == dtype
    return x, it, hist


def cg_half_epoch(mat, this, other, otor, tol, max_iter=0, dtype=np.float64, variant=None):
    "-> (factor rows [rows x k] in ``dtype``, iterations per row, ``frob_of`` them, r.r histories)"
    n_rows = mat.shape[0]
    k = other.shape[1]
    out = np.zeros((n_rows, k), dtype)
    its = np.zeros(n_rows, np.int64)
    hists = []
    for r in range(n_rows):
        s, e = mat.indptr[r], mat.indptr[r + 1]
        out[r], its[r], h = cg_row(other[mat.indices[s:e]], mat.data[s:e], otor, this[r], tol,
                                   max_iter, dtype, variant)
        hists.append(h)
    return out, its, frob_of(mat, out, this), hists


def frob_of(mat, new, old) -> float:
    """sqrt(sum ||new - old||^2) in float64 over the rows with entries: an empty row is zeroed and
    reports a delta of 0 (src/accel/als/implicit.rs:98-101), whatever it held before"""
    delta = (np.asarray(new, np.float64) - np.asarray(old, np.float64))[np.diff(mat.indptr) > 0]
    return float(np.sqrt(np.sum(delta * delta)))


def dense_solve(mat, other, otor):
    "-> (np.linalg.solve of every row's float64 system [rows x k], cond_2(A) per row; empty: 0, 1)"
    n_rows = mat.shape[0]
    x = np.zeros((n_rows, other.shape[1]))
    cond = np.ones(n_rows)
    for r in range(n_rows):
        s, e = mat.indptr[r], mat.indptr[r + 1]
        if e == s:
            continue
        A, y, _ = row_system(other[mat.indices[s:e]], mat.data[s:e], otor)
        x[r] = np.linalg.solve(A, y)
        ev = np.linalg.eigvalsh(A)
        assert ev[0] > 0
        cond[r] = ev[-1] / ev[0]
    return x, cond


# ---- the cases both test files share: computed once per process, read-only --------------------

KS = (33, 64, 65, 100, 128, 129, 200, 256)


def seed_of(k: int) -> int:
    "one seed per width (tests/test_als_cg_host.py asserts what the GPU tests need of it)"
    return 1000 + k


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(k: int, negative: bool = False):
    "the seam matrix of width k with its OtOr, row lengths and dense float64 answer"
    kp = padded(k)
    mat, other, this = seam_matrix(kp, seed_of(k), k, negative)
    otor = otor32(other)
    x, cond = dense_solve(mat, other, otor)
    lens = np.diff(mat.indptr)
    _frozen(mat.indptr, mat.indices, mat.data, other, this, otor, x, cond, lens)
    return types.SimpleNamespace(k=k, kp=kp, mat=mat, other=other, this=this, otor=otor, x=x,
                                 cond=cond, lens=lens, n_rows=mat.shape[0])


@functools.lru_cache(maxsize=None)
def fixed_iterations(k: int, negative: bool, m: int):
    "exactly m iterations from the warm start -> (float64 rows, float32 rows, per-row distance)"
    c = case(k, negative)
    x64, it64, _, _ = cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-20, m)
    x32, it32, _, _ = cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-20, m, np.float32)
    assert np.array_equal(it64, np.where(c.lens > 0, m, 0)) and np.array_equal(it32, it64)
    e = row_rel(x32, x64)
    _frozen(x64, x32, e)
    return x64, x32, e


@functools.lru_cache(maxsize=None)
def iteration_totals(k: int, negative: bool, tol: float, variant=None) -> int:
    "the float64 iteration total of a half-epoch at ``tol`` (max_iter = 2 k)"
    c = case(k, negative)
    return int(cg_half_epoch(c.mat, c.this, c.other, c.otor, tol, 2 * k, variant=variant)[1].sum())


def fixed_bound(e32_max: float) -> float:
    """what a float32 kernel may be from float64 after a fixed number of iterations: four times the
    float32 restatement's own distance (another summation order: four wave partials, the folded
    reduction, the fmaf chains) + 1e-6"""
    return 4.0 * e32_max + 1e-6


def converged_bound(cond, tol: float):
    "cond tol: the forward error of a relative residual tol; 16 cond u + 2e-6: the exact kernels' bound"
    return np.asarray(cond) * (tol + 16.0 * 2.0**-24) + 2e-6


def row_rel(a, b):
    "per-row ||a - b|| / ||b|| in float64 (rows with b = 0: the absolute distance)"
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.linalg.norm(b, axis=1)
    return np.linalg.norm(a - b, axis=1) / np.where(den > 0, den, 1.0)
