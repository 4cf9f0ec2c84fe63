#!/usr/bin/env python3
"""
Timing driver of the randomized SVD trainer (csrc/svd.hip) and ``BiasedSVDScorer`` on the device.

    python tools/svd_time.py [--out FILE] [--no-ml25m] [--no-host]

* accuracy, recorded next to the times: ``lk_chol_upper_inverse``'s residual
  ``|R^-T G R^-1 - I|max`` on Gramians of random 500 x l panels against float32
  ``numpy.linalg.cholesky``'s, and the distance of ``D.randomized_svd`` on the ml-latest-small
  bias residuals (k = 8 and 64, both orientations, the start panel of
  ``tests/golden/svd_ref.npz``) from the float64 restatement of ``tests/svd_restatement.py``,
  with the float32 restatement's own distance beside it.
* ml-latest-small and the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``)
  at k = 64, ``n_iter`` = 5: the fit (``D.randomized_svd`` on the residual matrix already in HBM,
  best of three after a warm-up), split into SpMM, orthonormalisation and the rest by a run with
  the stream synchronised around every step; SpMM bytes per second against the roofline
  ``nnz (4 ld + 8) + n_rows 4 ld`` bytes per pass; ``BiasedSVDScorer.train`` end to end (bias
  model, upload, transpose, fit, download); ``recommend_batch`` for 10 000 users, top-100.
* host scikit-learn ``TruncatedSVD`` (float32, as the reference calls it) on the same matrices, if
  scikit-learn imports; otherwise that it did not.
Times are host clocks around calls that end in a device synchronise.  One JSON document.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

K, N_ITER = 64, 5


def _residuals(ds):
    from lkpy_amd.basic import BiasModel

    bias = BiasModel.learn(ds, 5)
    mat = bias.transform_matrix(
        ds.interaction_matrix(format="scipy", layout="coo", field="rating")).tocsr()
    mat.sort_indices()
    mat.data = mat.data.astype(np.float32)
    return mat


def _accuracy(dev, ds):
    import scipy.linalg as sla
    import scipy.sparse as sps
    import torch

    import svd_restatement as R
    from lkpy_amd import _device as D

    out = {"chol_upper_inverse": [], "randomized_svd": []}
    for l in (11, 74, 138, 192):
        y = np.random.default_rng(l).normal(size=(500, l))
        g = (y.T @ y).astype(np.float32)
        g64 = g.astype(np.float64)
        resid = lambda t: float(np.abs(t.astype(np.float64) @ g64 @ t.T - np.eye(l)).max())  # noqa: E731
        t_np = sla.solve_triangular(np.linalg.cholesky(g), np.eye(l, dtype=np.float32), lower=True)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        inv, _ = D.chol_upper_inverse(torch.from_numpy(g).to(dev), flag, 1)
        out["chol_upper_inverse"].append({"l": l, "device": resid(inv.cpu().numpy()[:l, :l]),
                                          "numpy_float32": resid(t_np)})
    gold = np.load(ROOT / "tests" / "golden" / "svd_ref.npz")
    resid = _residuals(ds)
    for k in (8, 64):
        omega = gold["omega"][:, :k + R.OVERSAMPLES]
        for flipped in (False, True):
            a = sps.csr_array(resid.T) if flipped else resid
            a.sort_indices()
            f64 = R.randomized_svd(a, k, N_ITER, omega, np.float64)
            f32 = R.randomized_svd(a, k, N_ITER, omega, np.float32)
            csr = D.DeviceCSR.from_scipy(a, dev)
            got = D.randomized_svd(csr, D.csr_transpose(csr), k, N_ITER, omega)
            rng = np.random.default_rng(k)
            rows, cols = rng.integers(0, a.shape[0], 2000), rng.integers(0, a.shape[1], 2000)

            def dist(fit):
                s, comp, xt = (np.asarray(x, np.float64) for x in fit)
                rec = np.einsum("nk,kn->n", xt[rows], comp[:, cols])
                rec0 = np.einsum("nk,kn->n", f64[2][rows], f64[1][:, cols])
                return float(np.abs(s - f64[0]).max()), float(np.abs(rec - rec0).max())

            (ds_dev, dr_dev), (ds_32, dr_32) = dist(got), dist(f32)
            out["randomized_svd"].append({
                "k": k, "transposed_input": flipped, "shape": list(a.shape),
                "singular_values": {"device": ds_dev, "float32_restatement": ds_32},
                "reconstruction_2000_cells": {"device": dr_dev, "float32_restatement": dr_32}})
    return out


def _fit_times(resid, dev, reps=3):
    import torch

    from lkpy_amd import _device as D

    csr = D.DeviceCSR.from_scipy(resid, dev)
    csr_t = D.csr_transpose(csr)
    l = K + D.SVD_OVERSAMPLES
    ld = D.padded_dim(l)
    omega = np.random.default_rng(1).normal(size=(min(resid.shape), l))
    D.randomized_svd(csr, csr_t, K, 1, omega, device_output=True)  # warm-up
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.randomized_svd(csr, csr_t, K, N_ITER, omega, device_output=True)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    stats: dict = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D.randomized_svd(csr, csr_t, K, N_ITER, omega, device_output=True, stats=stats)
    stepped = time.perf_counter() - t0
    # the roofline's bytes: every pass over the sketch panels (the last SpMM has the k-wide panel)
    n_rows, n_cols = resid.shape
    passes = stats["spmm_calls"] - 1
    per_pair = 2 * resid.nnz * (4 * ld + 8) + (n_rows + n_cols) * 4 * ld
    kd = D.padded_dim(K)
    sketch_bytes = passes // 2 * per_pair
    last_bytes = resid.nnz * (4 * kd + 8) + n_rows * 4 * kd
    return {
        "k": K, "n_iter": N_ITER, "l": l, "ld": ld, "shape": [n_rows, n_cols],
        "nnz": int(resid.nnz), "fit_seconds": round(min(walls), 6),
        "fit_seconds_all": [round(w, 6) for w in walls],
        "stepped_run": {
            "what": "one fit with the stream synchronised around every step",
            "seconds": round(stepped, 6), "spmm_seconds": round(stats["spmm"], 6),
            "orth_seconds": round(stats["orth"], 6),
            "rest_seconds": round(stepped - stats["spmm"] - stats["orth"], 6),
            "spmm_calls": stats["spmm_calls"], "orth_calls": stats["orth_calls"]},
        "spmm_roofline_bytes": int(sketch_bytes + last_bytes),
        "spmm_gb_per_s": round((sketch_bytes + last_bytes) / stats["spmm"] / 1e9, 1),
    }


def _host_sklearn(resid):
    try:
        from sklearn.decomposition import TruncatedSVD
    except Exception as e:  # noqa: BLE001
        return {"imported": False, "error": f"{type(e).__name__}: {e}"}
    import sklearn

    t0 = time.perf_counter()
    TruncatedSVD(K, algorithm="randomized", n_iter=N_ITER, random_state=1).fit_transform(resid)
    return {"imported": True, "version": sklearn.__version__, "dtype": str(resid.dtype),
            "fit_transform_seconds": round(time.perf_counter() - t0, 3)}


def _component(ds, reps=3):
    import torch

    from lkpy_amd.basic import UserTrainingHistoryLookup
    from lkpy_amd.sklearn.svd import BiasedSVDScorer
    from lkpy_amd.training import TrainingOptions

    sc = BiasedSVDScorer(features=K)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc.train(ds, TrainingOptions(rng=1))
    t_train = time.perf_counter() - t0
    lookup = UserTrainingHistoryLookup()
    lookup.train(ds)
    n = min(10000, ds.user_count)
    users = np.random.default_rng(43).choice(ds.user_count, n, replace=False)
    uids = ds.users.ids()[users]
    sc.recommend_batch(lookup.batch(uids[:256]), 100)  # uploads
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.recommend_batch(lookup.batch(uids), 100)
        ts.append(time.perf_counter() - t0)
    return {"train_seconds": round(t_train, 4),
            "train_what": "BiasedSVDScorer.train: bias model (on the device), upload, transpose, "
                          "fit, download",
            "recommend": {"users": int(n), "n": 100, "seconds": round(min(ts), 5),
                          "seconds_all": [round(t, 5) for t in ts],
                          "users_per_s": round(n / min(ts), 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "spmm_split": D.spmm_split(),
           "chol_max_l": D.chol_max_l()}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    res["accuracy"] = _accuracy(dev, ds)
    emit()
    resid = _residuals(ds)
    small = _fit_times(resid, dev)
    small.update(_component(ds))
    if not args.no_host:
        small["host_sklearn"] = _host_sklearn(resid)
    res["ml_latest_small"] = small
    emit()

    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        dset = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                       Vocabulary(np.arange(n_i), "item", reorder=False),
                       rows, ratings.indices, {"rating": ratings.data})
        resid = _residuals(dset)
        big = _fit_times(resid, dev)
        res["ml25m_like"] = big
        emit()
        big.update(_component(dset))
        emit()
        if not args.no_host:
            big["host_sklearn"] = _host_sklearn(resid)
    print(emit())


if __name__ == "__main__":
    main()
