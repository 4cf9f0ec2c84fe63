"""
NumPy restatement of ``lk_spd_inverse_blocked`` (csrc/spd_blocked.hip) and of what
``EASEScorer.train`` makes of it: the same block steps in the same order, float32 GEMMs for the
panels, the trailing updates and the products, the diagonal block factored and inverted with
float64 sums rounded once (``lk_chol_upper_inverse``).  A float32 NumPy GEMM sums in another order
than the k-ordered MFMA chain, so the device is not expected to match this bit for bit: both are
held to the same distance from the float64 inverse.  Shared by the host and the GPU tests.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sps

NB = 128  # lk_gemm_tile(): the block size of the factorisation
TINY = np.float32(4.0 * 2.0 ** -24)  # a pivot at or below 4 ulp of its diagonal entry is noise


def chol_lower_inverse(g: np.ndarray):
    """
    ``lk_chol_upper_inverse`` on one diagonal block: (L, L^-1, failed).  float32 entries, every
    sum behind an entry carried in float64 and rounded once; a pivot that is not positive to
    working precision is replaced by the block's diagonal entry (1 if that is not positive either).
    """
    l = g.shape[0]
    low = np.zeros((l, l), dtype=np.float32)
    failed = False
    for j in range(l):
        s = g[j:, j].astype(np.float64) - low[j:, :j].astype(np.float64) @ \
            low[j, :j].astype(np.float64)
        d = s[0]
        gjj = g[j, j]
        if not (np.float32(d) > TINY * gjj) or not np.isfinite(np.float32(d)):
            failed = True
            d = float(gjj) if (gjj > 0 and np.isfinite(gjj)) else 1.0
        ljj = np.float32(np.sqrt(d))
        col = (s / np.float64(ljj)).astype(np.float32)
        col[~np.isfinite(col)] = 0.0
        low[j:, j] = col
        low[j, j] = ljj
    dinv = 1.0 / np.diag(low).astype(np.float64)
    inv = np.zeros((l, l), dtype=np.float32)
    low64 = low.astype(np.float64)
    for j in range(l):  # column j of L^-1 by forward substitution
        x = np.zeros(l, dtype=np.float32)
        x[j] = np.float32(dinv[j])
        for i in range(j + 1, l):
            s = low64[i, j:i] @ x[j:i].astype(np.float64)
            x[i] = np.float32(-s * dinv[i])
        inv[:, j] = x
    return low, inv, failed


def spd_inverse_blocked(a: np.ndarray, nb: int = NB):
    """
    (inverse, flag) of the SPD matrix ``a`` by the device's block steps: flag = 0, or 1 + the first
    block whose factorisation met a pivot that is not positive -- the inverse is then zeros.
    """
    a = np.array(a, dtype=np.float32)
    n = a.shape[0]
    blocks = [(r0, min(n, r0 + nb)) for r0 in range(0, n, nb)]
    low = np.zeros((n, n), dtype=np.float32)  # L's off-diagonal blocks (the device's W)
    dinv = []
    flag = 0
    with np.errstate(all="ignore"):
        # (a) right-looking Cholesky
        for j, (r0, r1) in enumerate(blocks):
            _l, inv, failed = chol_lower_inverse(a[r0:r1, r0:r1])
            if failed and flag == 0:
                flag = j + 1
            dinv.append(inv)
            if r1 < n:
                p = a[r1:, r0:r1] @ inv.T
                low[r1:, r0:r1] = p
                a[r1:, r1:] -= p @ p.T
        # (b) X = L^-1, block row by block row
        x = np.zeros((n, n), dtype=np.float32)
        for i, (r0, r1) in enumerate(blocks):
            x[r0:r1, r0:r1] = dinv[i]
            if r0:
                t = low[r0:r1, :r0] @ x[:r0, :r0]
                x[r0:r1, :r0] = -(dinv[i] @ t)
        # (c) X^T X on the lower triangle, mirrored
        out = np.tril(x.T @ x)
        out = out + np.tril(out, -1).T
    if flag:
        out = np.zeros((n, n), dtype=np.float32)
    return out, flag


def ease_gramian(ui, reg: float) -> np.ndarray:
    "``X^T X + reg I`` (float32, exact integer counts) of the binary users x items matrix."
    x = sps.csr_array(ui, dtype=np.float32)
    x.sum_duplicates()
    x.data[:] = 1.0
    g = np.asarray((x.T @ x).todense(), dtype=np.float32)
    g[np.diag_indices(g.shape[0])] += np.float32(reg)
    return g


def ease_weights(inv: np.ndarray) -> np.ndarray:
    "``B = inv / -diag(inv)`` with a zero diagonal (ease.py:140-142), in ``inv``'s precision."
    mat = inv / -np.diag(inv).reshape(1, -1)
    mat[np.diag_indices(mat.shape[0])] = 0
    return mat


def lapack_inverse_f32(g: np.ndarray) -> np.ndarray:
    "The oracle's path on the Gramian alone: LAPACK ``spotrf`` + ``spotri`` in float32."
    import scipy.linalg as spla

    c, info = spla.lapack.spotrf(np.array(g, dtype=np.float32), lower=1)
    assert info == 0
    mat, info = spla.lapack.spotri(c, lower=1)
    assert info == 0
    return np.tril(mat) + np.tril(mat, -1).T


def rel_dist(x: np.ndarray, ref: np.ndarray) -> float:
    "Relative Frobenius distance from the float64 reference."
    return float(np.linalg.norm(x.astype(np.float64) - ref) / np.linalg.norm(ref))


def top_items_matrix(ml_small: dict, n_items: int) -> sps.csr_array:
    "The binary ml-latest-small matrix restricted to its ``n_items`` most-rated items."
    rmat = sps.csr_array(ml_small["rmat"])
    counts = np.diff(sps.csc_array(rmat).indptr)
    top = np.sort(np.argsort(-counts, kind="stable")[:n_items])
    return sps.csr_array(rmat[:, top])


def indefinite_second_block(n: int = 200) -> np.ndarray:
    "An SPD-looking matrix whose second diagonal block (rows 128 ...) has a negative pivot."
    rng = np.random.default_rng(7)
    b = rng.standard_normal((n, n + 20)).astype(np.float32)
    g = (b @ b.T + np.float32(n) * np.eye(n, dtype=np.float32)).astype(np.float32)
    g[NB + 5, NB + 5] = np.float32(-3.0)
    return g
