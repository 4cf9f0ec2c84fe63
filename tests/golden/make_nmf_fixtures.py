#!/usr/bin/env python3
"""Pin the NMF restatement to scikit-learn's ``non_negative_factorization``, executed here.

``NMFScorer.train`` of the reference (src/lenskit/sklearn/nmf.py:72-110) hands the float32
indicator matrix to ``sklearn.decomposition.non_negative_factorization``: the NNDSVDA start and
Frobenius coordinate descent in float32.  This script runs scikit-learn and records what
``tests/test_nmf_host.py`` and ``tests/test_gpu_nmf.py`` compare against:

    python tests/golden/make_nmf_fixtures.py        ->  tests/golden/nmf_ref.npz

Two random binary matrices (density 0.15, seed 20250714: from 20250713 the unregularised fit
runs into ``max_iter``, and the tests want one that stops by ``tol``), each with the start
sklearn's own ``_initialize_nmf(init="nndsvda", random_state=0)`` gives it, fitted from that
start (``init="custom"``) at the default ``tol`` and ``max_iter``:

    a_*: 60 x 90, k = 5, no regularisation
    b_*: 200 x 150, k = 16, ``alpha_W=0.01, l1_ratio=0.5``

stored as the matrix (dense uint8), ``w0`` / ``h0``, sklearn's ``w`` / ``h`` and ``n_iter``.

ml-latest-small as an indicator matrix (671 x 9125), k = 8: ``_initialize_nmf`` with its
``_randomized_svd`` replaced by the float64 restatement's ``U, S, V`` (``svd_restatement``, 7 power
iterations from the first 18 columns of ``svd_ref.npz["omega"]``) rounded to float32 -- ``ml_u``,
``ml_s``, ``ml_v`` are those inputs, ``ml_w0`` / ``ml_h0`` sklearn's start -- and 10 sweeps from
it at ``tol=0``: ``ml_recon10`` is ``W H`` at the 2 000 cells (``ml_rows``, ``ml_cols``).
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import scipy.sparse as sps
import sklearn.decomposition._nmf as sk_nmf
from sklearn.decomposition import non_negative_factorization

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parent.parent))
import nmf_restatement as R  # noqa: E402

SEED = 20250714
CASES = {"a": dict(shape=(60, 90), k=5, alpha_W=0.0, l1_ratio=0.0),
         "b": dict(shape=(200, 150), k=16, alpha_W=0.01, l1_ratio=0.5)}


def main():
    from lkpy_amd.data import load_movielens_npz

    warnings.simplefilter("ignore")  # ConvergenceWarning of the tol=0 run
    rng = np.random.default_rng(SEED)
    out = dict(seed=SEED)
    for name, c in CASES.items():
        x = (rng.random(c["shape"]) < 0.15).astype(np.float32)
        w0, h0 = sk_nmf._initialize_nmf(x, c["k"], init="nndsvda", random_state=0)
        assert w0.dtype == np.float32
        w, h, n_iter = non_negative_factorization(
            sps.csr_array(x), W=w0.copy(), H=h0.copy(), n_components=c["k"], init="custom",
            alpha_W=c["alpha_W"], l1_ratio=c["l1_ratio"])
        assert w.dtype == np.float32
        l1_w, l1_h, l2_w, l2_h = (x.shape[1] * c["alpha_W"] * c["l1_ratio"],
                                  x.shape[0] * c["alpha_W"] * c["l1_ratio"],
                                  x.shape[1] * c["alpha_W"] * (1 - c["l1_ratio"]),
                                  x.shape[0] * c["alpha_W"] * (1 - c["l1_ratio"]))
        rw, rh, rn, _ = R.fit(x, w0, h0, 200, 1e-4, l1_w, l1_h, l2_w, l2_h, np.float32, "sklearn")
        print(f"{name}: sklearn n_iter {n_iter}, restatement {rn}; W equal "
              f"{np.array_equal(rw, w)}, H equal {np.array_equal(rh, h)}")
        out.update({f"{name}_x": x.astype(np.uint8), f"{name}_w0": w0, f"{name}_h0": h0,
                    f"{name}_w": w, f"{name}_h": h, f"{name}_n_iter": n_iter,
                    f"{name}_alpha_W": c["alpha_W"], f"{name}_l1_ratio": c["l1_ratio"]})

    ds = load_movielens_npz(OUT / "ml_small.npz")
    x = ds.interactions().matrix().scipy(layout="csr").astype(np.float32)
    k = 8
    omega = np.load(OUT / "svd_ref.npz")["omega"][:, :k + 10]
    s, comp, xt = R.randomized_svd(x, k, 7, omega, np.float64)
    u32, s32, v32 = (xt / s).astype(np.float32), s.astype(np.float32), comp.astype(np.float32)
    real_svd = sk_nmf._randomized_svd
    sk_nmf._randomized_svd = lambda *a, **kw: (u32, s32, v32)
    try:
        w0, h0 = sk_nmf._initialize_nmf(x, k, init="nndsvda")
    finally:
        sk_nmf._randomized_svd = real_svd
    rw0, rh0 = R.nndsvda(u32, s32, v32, x.mean(), np.float32)
    print(f"ml_small start: restatement vs sklearn: W {np.abs(rw0 - w0).max():.1e}, "
          f"H {np.abs(rh0 - h0).max():.1e}")
    w, h, n_iter = non_negative_factorization(x, W=w0.copy(), H=h0.copy(), n_components=k,
                                              init="custom", tol=0.0, max_iter=10)
    rows = rng.integers(0, x.shape[0], 2000).astype(np.int32)
    cols = rng.integers(0, x.shape[1], 2000).astype(np.int32)
    rw, rh, _, _ = R.fit(x, w0, h0, 10, 0.0, dtype=np.float32)
    print(f"ml_small 10 sweeps: W equal {np.array_equal(rw, w)}, H equal {np.array_equal(rh, h)}")
    out.update(ml_u=u32, ml_s=s32, ml_v=v32, ml_w0=w0, ml_h0=h0, ml_rows=rows, ml_cols=cols,
               ml_recon10=R.recon(w, h, rows, cols), ml_n_iter=n_iter)
    path = OUT / "nmf_ref.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
