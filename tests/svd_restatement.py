"""
NumPy / SciPy restatement of the randomized truncated SVD the device trainer runs
(``lkpy_amd._device.randomized_svd``) and of ``BiasedSVDScorer.__call__``'s arithmetic.

The algorithm is sklearn's ``randomized_svd`` / ``randomized_range_finder`` as
``TruncatedSVD.fit_transform`` calls them (``n_oversamples = 10``, ``transpose="auto"``, the
Gaussian start panel given), with one substitution: the normaliser between the products is
CholeskyQR2 (Gramian -> Cholesky factor -> multiply by its inverse, twice) where sklearn uses LU
in the power iterations and QR at the end.  The result depends on the RANGE of the sketch only,
so in float64 this reproduces sklearn to 1e-13 (``tests/test_svd_host.py`` holds it to the
golden file).  ``dtype=np.float32`` runs every step in float32, as the device does; its distance
from the float64 run is the yardstick the device tests use.
"""

from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

OVERSAMPLES = 10


def chol_qr(y: np.ndarray):
    "One CholeskyQR pass: (Q, R) with Y = Q R, R upper triangular, in Y's dtype."
    dt = y.dtype
    gram = (y.T @ y).astype(dt)
    r = np.linalg.cholesky(gram).T.astype(dt)
    r_inv = sla.solve_triangular(r, np.eye(len(r), dtype=dt), lower=False).astype(dt)
    return (y @ r_inv).astype(dt), r


def orth(y: np.ndarray):
    "CholeskyQR2: (Q, R) with Y = Q R; the second pass repairs the first's loss of orthogonality."
    q1, r1 = chol_qr(y)
    q2, r2 = chol_qr(q1)
    return q2, (r2 @ r1).astype(y.dtype)


def svd_flip_v(components: np.ndarray) -> np.ndarray:
    "``svd_flip(u_based_decision=False)``: each row's largest-magnitude entry made positive."
    rows = np.arange(components.shape[0])
    signs = np.sign(components[rows, np.argmax(np.abs(components), axis=1)])
    signs[signs == 0] = 1
    return components * signs[:, None]


def operates_on_transpose(shape) -> bool:
    "sklearn's ``transpose='auto'``"
    return shape[0] < shape[1]


def randomized_svd(a, k: int, n_iter: int, omega: np.ndarray, dtype=np.float64):
    """
    (singular_values [k], components [k x n_cols], transformed [n_rows x k]) of the sparse matrix
    ``a`` from the start panel ``omega`` [min(shape) x (k + 10)], every step in ``dtype``.
    """
    a = sps.csr_array(a).astype(dtype)
    l = k + OVERSAMPLES
    if l > min(a.shape):
        raise ValueError(f"k + {OVERSAMPLES} = {l} exceeds the matrix's smaller dimension")
    transpose = operates_on_transpose(a.shape)
    m = sps.csr_array(a.T) if transpose else a  # tall: m.shape[0] >= m.shape[1]
    mt = sps.csr_array(m.T)
    q = np.asarray(omega, dtype=dtype)
    assert q.shape == (m.shape[1], l), (q.shape, m.shape, l)
    for _ in range(n_iter):
        q, _ = orth(np.asarray(m @ q, dtype=dtype))
        q, _ = orth(np.asarray(mt @ q, dtype=dtype))
    q, _ = orth(np.asarray(m @ q, dtype=dtype))
    bt = np.asarray(mt @ q, dtype=dtype)  # B^T = M^T Q
    q_b, r_b = orth(bt)
    # the one step that is float64 whatever the dtype: the SVD of the l x l factor
    w, s, zt = sla.svd(r_b.astype(np.float64), lapack_driver="gesdd")
    # B = Z S (Q_b W)^T: left vectors of M are Q Z, right vectors Q_b W
    if transpose:
        v = (q @ zt.T[:, :k].astype(dtype)).astype(dtype)  # right vectors of A = left of M
    else:
        v = (q_b @ w[:, :k].astype(dtype)).astype(dtype)
    components = svd_flip_v(v.T).astype(dtype)
    transformed = np.asarray(a @ components.T, dtype=dtype)
    return s[:k], components, transformed


def bias_residuals(rows, cols, vals, shape, damping: float):
    """
    ``BiasModel.learn`` + ``transform_matrix`` (src/lenskit/basic/bias.py:83-150, 246-275) on raw
    triples, in the dtypes the package's own ``BiasModel`` works in: the ratings stay float32,
    the sums are float64, the biases float32.  Returns (global bias, item biases, user biases,
    the residuals as float32 CSR).
    """
    vals = np.asarray(vals)
    g = float(np.mean(vals))
    centred = vals - g
    counts = np.full(shape[1], float(damping))
    sums = np.zeros(shape[1])
    np.add.at(counts, cols, 1)
    np.add.at(sums, cols, centred)
    ib = np.zeros(shape[1], dtype=np.float32)
    np.divide(sums, counts, out=ib, where=counts > 0)
    centred = centred - ib[cols]
    counts = np.full(shape[0], float(damping))
    sums = np.zeros(shape[0])
    np.add.at(counts, rows, 1)
    np.add.at(sums, rows, centred)
    ub = np.zeros(shape[0], dtype=np.float32)
    np.divide(sums, counts, out=ub, where=counts > 0)
    resid = vals - g
    resid -= ib[cols]
    resid -= ub[rows]
    mat = sps.csr_array(sps.coo_array((resid.astype(np.float32), (rows, cols)), shape=shape))
    mat.sort_indices()
    return g, ib, ub, mat


def score(user_components_row, components, item_nums, global_bias, item_biases, user_bias,
          dtype=np.float64):
    """
    ``BiasedSVDScorer.__call__`` for known items: ``inverse_transform`` of the user's row at the
    items, plus global + item + user bias.  float32: the device's arithmetic (every term float32).
    """
    x = np.asarray(user_components_row, dtype=dtype)
    v = np.asarray(components, dtype=dtype)[:, item_nums]
    out = (x @ v).astype(dtype)
    out = out + dtype(global_bias)
    out = out + np.asarray(item_biases, dtype=dtype)[item_nums]
    return (out + dtype(user_bias)).astype(dtype)
