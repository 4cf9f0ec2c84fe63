#!/usr/bin/env python3
"""
Timing driver of the NMF trainer (csrc/nmf.hip, ``lkpy_amd._device.nmf_fit``) on the device.

    python tools/nmf_time.py [--out FILE] [--iters N] [--small] [--no-host]

On the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``) as an indicator
matrix, k = 64 (``--small``: ml-latest-small instead):

* the start: the randomized SVD on the device (7 or 4 power iterations, as sklearn's "auto") and
  NNDSVDA on the host, each on its own clock;
* ``--iters`` (default 5) iterations of the fit at ``tol=0``: the wall time, and from a second run
  with the stream synchronised around every step the seconds per iteration in the Gramian
  (``lk_gramian``), the sparse product (``lk_csr_spmm``) and the sweep (``lk_nmf_cd_sweep``), the
  sweep's share of them, and the sweep's arithmetic rate (2 k^2 flops a row);
* host scikit-learn's ``non_negative_factorization`` (float32, as the reference calls it) from
  the same start for the same iterations, if scikit-learn imports; otherwise that it did not.
Times are host clocks around calls that end in a device synchronise.  One JSON document.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K = 64


def _host_sklearn(mat, w0, h0, iters):
    try:
        from sklearn.decomposition import non_negative_factorization
    except Exception as e:  # noqa: BLE001
        return {"imported": False, "error": f"{type(e).__name__}: {e}"}
    import sklearn

    warnings.simplefilter("ignore")  # the ConvergenceWarning of a tol=0 run
    t0 = time.perf_counter()
    non_negative_factorization(mat, W=w0.copy(), H=h0.copy(), n_components=K, init="custom",
                               tol=0.0, max_iter=iters)
    wall = time.perf_counter() - t0
    return {"imported": True, "version": sklearn.__version__, "dtype": str(mat.dtype),
            "iterations": iters, "seconds": round(wall, 3),
            "seconds_per_iteration": round(wall / iters, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.sklearn.nmf import nndsvda

    dev = D.device()
    if args.small:
        from lkpy_amd.data import load_movielens_npz

        ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
        mat = ds.interactions().matrix().scipy(layout="csr").astype(np.float32)
    else:
        from lkpy_amd import synth

        mat = synth.ml25m_like().astype(np.float32)
        mat.data[:] = 1
    mat.sort_indices()
    n_rows, n_cols = mat.shape
    res = {"device": torch.cuda.get_device_name(dev), "k": K, "shape": [n_rows, n_cols],
           "nnz": int(mat.nnz), "nmf_max_k": D.nmf_max_k()}

    csr = D.DeviceCSR.from_arrays(mat.indptr, mat.indices, mat.data, mat.shape, dev)
    csr_t = D.csr_transpose(csr)
    n_iter = 7 if K < 0.1 * min(mat.shape) else 4
    omega = np.random.default_rng(1).normal(size=(min(mat.shape), K + D.SVD_OVERSAMPLES))
    D.randomized_svd(csr, csr_t, K, 1, omega)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sv, comp, xt = D.randomized_svd(csr, csr_t, K, n_iter, omega)
    t_svd = time.perf_counter() - t0
    t0 = time.perf_counter()
    s32 = sv.astype(np.float32)
    w0, h0 = nndsvda((xt / s32).astype(np.float32), s32, comp, mat.mean())
    t_nnd = time.perf_counter() - t0
    res["start"] = {"svd_power_iterations": n_iter, "svd_seconds": round(t_svd, 4),
                    "nndsvda_host_seconds": round(t_nnd, 4)}

    D.nmf_fit(csr, csr_t, w0, h0, 1, 0.0)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, done, hist = D.nmf_fit(csr, csr_t, w0, h0, args.iters, 0.0)
    wall = time.perf_counter() - t0
    stats: dict = {}
    D.nmf_fit(csr, csr_t, w0, h0, args.iters, 0.0, stats=stats)
    steps = {key: stats[key] / done for key in ("gramian", "spmm", "sweep")}
    total = sum(steps.values())
    res["fit"] = {
        "iterations": int(done), "seconds": round(wall, 4),
        "seconds_per_iteration": round(wall / done, 5),
        "what": "nmf_fit: upload of the start, the iterations, download of the factors",
        "stepped_run_seconds_per_iteration": {key: round(v, 6) for key, v in steps.items()},
        "sweep_share_of_steps": round(steps["sweep"] / total, 4),
        "sweep_gflop_per_s": round(2.0 * K * K * (n_rows + n_cols) / steps["sweep"] / 1e9, 1),
        "violation_ratio_last": float(hist[-1] / hist[0])}
    if not args.no_host:
        res["host_sklearn"] = _host_sklearn(mat, w0, h0, args.iters)
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
