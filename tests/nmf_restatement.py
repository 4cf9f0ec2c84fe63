"""
NumPy restatement of the NMF trainer (``lkpy_amd._device.nmf_fit``, ``lkpy_amd.sklearn.nmf``):
sklearn's Frobenius coordinate descent (``_fit_coordinate_descent`` / ``_update_cdnmf_fast``) and
its NNDSVDA start (``_initialize_nmf``, ``_nmf.py:317-361``), every step in a given dtype.

In float32 the sweep gives sklearn's bits: NumPy rounds a product and a sum separately, as the C
loop sklearn compiles does, and the rows are independent, so running the coordinates ``t`` for
all rows at once changes nothing.  ``dtype=np.float64`` is the yardstick: the distance of the
float32 run from it is what the device tests allow the device (times four).

The violation is summed two ways: ``"sklearn"`` is sklearn's own sum -- in the working dtype,
sequentially, coordinate by coordinate and row by row inside one (``np.cumsum`` is sequential) --
which decides sklearn's stopping iteration; ``"float64"`` is the float64 sum of the same terms,
which is what the device forms (in another order).
"""

from __future__ import annotations

from math import sqrt

import numpy as np
import scipy.sparse as sps

from svd_restatement import randomized_svd  # noqa: F401  (the start's SVD, re-exported)

EPS = 1e-6  # ``_initialize_nmf``'s ``eps``
BAND = (0.5e-6, 2e-6)  # values this close to EPS may fall on either side of it in float32


def sweep(w: np.ndarray, hht: np.ndarray, xht: np.ndarray, l1_reg: float = 0.0):
    """
    One ``_update_cdnmf_fast`` pass over ``w`` [n x k] in place, in ``w``'s dtype; ``xht`` is
    ``X Ht`` before ``l1_reg`` is taken off.  Returns ``|pg|`` [n x k].
    """
    dt = w.dtype.type
    n, k = w.shape
    hht = np.asarray(hht, dtype=dt)
    x = (np.asarray(xht, dtype=dt) - dt(l1_reg)).astype(dt)
    pg_abs = np.zeros((n, k), dtype=dt)
    zero = dt(0)
    for t in range(k):
        grad = -x[:, t]
        for r in range(k):
            grad = grad + hht[t, r] * w[:, r]
        pg = np.where(w[:, t] == 0, np.where(grad < 0, grad, zero), grad)
        pg_abs[:, t] = np.abs(pg)
        hess = hht[t, t]
        if hess != 0:
            v = w[:, t] - grad / hess
            w[:, t] = np.where(v > 0, v, zero)
    return pg_abs


def violation(pg_abs: np.ndarray, how: str = "float64") -> float:
    "The sum of a sweep's ``|pg|``: sklearn's sequential sum in the dtype, or a float64 sum."
    if pg_abs.size == 0:
        return 0.0
    if how == "sklearn":  # coordinate t outside, row i inside
        return float(np.cumsum(pg_abs.T.ravel(), dtype=pg_abs.dtype)[-1])
    return float(pg_abs.astype(np.float64).sum())


def half(x, w, ht, l1_reg, l2_reg):
    "``_update_coordinate_descent``: the Gramian, the product, the sweep of ``w``; -> ``|pg|``"
    dt = w.dtype.type
    hht = (ht.T @ ht).astype(dt)
    if l2_reg != 0.0:
        hht.flat[:: hht.shape[0] + 1] += dt(l2_reg)
    xht = np.asarray(x @ ht, dtype=dt)
    return sweep(w, hht, xht, l1_reg)


def fit(x, w0, h0, max_iter: int, tol: float, l1_w=0.0, l1_h=0.0, l2_w=0.0, l2_h=0.0,
        dtype=np.float32, how: str = "float64"):
    "``_fit_coordinate_descent``: (W, H, n_iter, the violations of the iterations run)"
    x = sps.csr_array(x).astype(dtype)
    xt = sps.csr_array(x.T)
    w = np.array(w0, dtype=dtype, order="C")
    ht = np.array(np.asarray(h0).T, dtype=dtype, order="C")
    history = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        v = violation(half(x, w, ht, l1_w, l2_w), how)
        v += violation(half(xt, ht, w, l1_h, l2_h), how)
        history.append(v)
        if history[0] == 0 or v / history[0] <= tol:
            break
    return w, np.ascontiguousarray(ht.T), n_iter, np.asarray(history)


def _norm(x) -> float:
    "sklearn's ``norm``: ``math.sqrt`` of the dot product in the vector's dtype"
    return sqrt(np.dot(x, x))


def nndsvd_raw(u, s, v, dtype=np.float64):
    "``_nmf.py:318-353``: (W, H) before the ``< eps`` threshold, from ``U, S, V`` in ``dtype``"
    U, S, V = (np.asarray(a, dtype=dtype) for a in (u, s, v))
    W = np.zeros_like(U)
    H = np.zeros_like(V)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, len(S)):
        x, y = U[:, j], V[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = _norm(x_p), _norm(y_p)
        x_n_nrm, y_n_nrm = _norm(x_n), _norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            uu = x_p / x_p_nrm
            vv = y_p / y_p_nrm
            sigma = m_p
        else:
            uu = x_n / x_n_nrm
            vv = y_n / y_n_nrm
            sigma = m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * uu
        H[j, :] = lbd * vv
    return W, H


def choice_margins(u, s, v) -> np.ndarray:
    "``|m_p - m_n| / max(m_p, m_n)`` of the components 1 .. k-1 in float64"
    U, V = np.asarray(u, np.float64), np.asarray(v, np.float64)
    out = []
    for j in range(1, U.shape[1]):
        m_p = _norm(np.maximum(U[:, j], 0)) * _norm(np.maximum(V[j], 0))
        m_n = _norm(np.minimum(U[:, j], 0)) * _norm(np.minimum(V[j], 0))
        out.append(abs(m_p - m_n) / max(m_p, m_n))
    return np.asarray(out)


def threshold_fill(raw: np.ndarray, avg, flip: np.ndarray | None = None) -> np.ndarray:
    """``_nmf.py:355-361``: values below ``eps`` become 0 and every 0 becomes ``avg``; the cells
    of the mask ``flip`` are forced to the other side of the threshold."""
    below = raw < EPS
    if flip is not None:
        below = below ^ flip
    out = raw.copy()
    out[below | (raw == 0)] = avg
    return out


def band(raw: np.ndarray) -> np.ndarray:
    "the cells whose value before the threshold lies in ``BAND``"
    return (raw >= BAND[0]) & (raw <= BAND[1])


def nndsvda(u, s, v, avg, dtype=np.float64):
    "The NNDSVDA start (W [n x k], H [k x m]) from ``U, S, V`` and ``avg = X.mean()``"
    W, H = nndsvd_raw(u, s, v, dtype)
    avg = np.asarray(avg, dtype=dtype)[()]
    return threshold_fill(W, avg), threshold_fill(H, avg)


def start(x, k: int, omega, dtype=np.float64):
    """The whole start as the component forms it: the randomized SVD (7 power iterations below a
    tenth of the smaller dimension, else 4), ``U = transformed / s``, NNDSVDA.  Returns
    (W0, H0, the values before the threshold (W, H))."""
    x = sps.csr_array(x).astype(dtype)
    n_iter = 7 if k < 0.1 * min(x.shape) else 4
    s, comp, xt = randomized_svd(x, k, n_iter, omega, dtype)
    s = s.astype(dtype)
    u = (xt / s).astype(dtype)
    raw_w, raw_h = nndsvd_raw(u, s, comp, dtype)
    avg = np.asarray(x.mean(), dtype=dtype)[()]
    return threshold_fill(raw_w, avg), threshold_fill(raw_h, avg), (raw_w, raw_h)


def loss(x, w, h) -> float:
    "``0.5 ||X - W H||^2`` in float64 without forming ``W H``: X is sparse"
    x = sps.csr_array(x).astype(np.float64)
    w, h = np.asarray(w, np.float64), np.asarray(h, np.float64)
    wh2 = float(np.sum((w.T @ w) * (h @ h.T)))
    cross = float(np.sum(np.asarray(x @ h.T) * w))
    return 0.5 * (float(x.multiply(x).sum()) - 2.0 * cross + wh2)


def recon(w, h, rows, cols) -> np.ndarray:
    "``(W H)[rows, cols]`` in float64"
    return np.einsum("ij,ji->i", np.asarray(w, np.float64)[rows],
                     np.asarray(h, np.float64)[:, cols])
