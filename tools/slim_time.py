#!/usr/bin/env python3
"""
Timing driver of the SLIM / fsSLIM trainer and scorer (csrc/slim.hip) on the device.

    python tools/slim_time.py [--out FILE] [--no-ml25m] [--sample N] [--full-limit SECONDS]

* ml-latest-small (tests/golden/ml_small.npz): the whole fit at the default configuration and at
  ``max_nbrs = 500``, three runs each after a warm-up, with the descent's own counts (rounds,
  coordinate updates, residual entries summed) so that every time has a rate next to it.
* the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``) at
  ``max_nbrs = 500``: a seeded uniform sample of columns first; the whole fit when the sample's
  rate predicts it under ``--full-limit`` seconds (otherwise the extrapolation is reported, named
  as such); then ``batch.recommend``-shaped scoring, 10 000 users, top-100.
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


def _pair(csr, dev):
    import scipy.sparse as sps
    import torch

    from lkpy_amd import _device as D

    ui = sps.csr_array(csr)
    ui.sort_indices()
    iu = sps.csr_array(ui.T)
    iu.sort_indices()

    def up(m):
        h = m.indptr.astype(np.int32 if m.nnz < 2 ** 31 - 64 else np.int64)
        return D.DeviceCSR(torch.from_numpy(h).to(dev),
                           torch.from_numpy(m.indices.astype(np.int32)).to(dev), None,
                           (int(m.shape[0]), int(m.shape[1])), h)

    return up(ui), up(iu)


def _fit(ui, iu, cfg, columns=None, reps=1):
    import torch

    from lkpy_amd import _device as D

    walls, stats, nnz = [], {}, 0
    for _ in range(reps):
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = D.slim_train(ui, iu, *cfg, columns=columns, stats=stats)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        nnz = out.nnz
        del out
    best = min(walls)
    return {"config": {"l1_reg": cfg[0], "l2_reg": cfg[1], "max_iters": cfg[2],
                       "max_nbrs": cfg[3]},
            "columns": int(ui.shape[1] if columns is None else len(columns)),
            "seconds": round(best, 5), "seconds_all": [round(w, 5) for w in walls],
            "weights": int(nnz), **stats,
            "resid_entries_per_s": round(stats["resid_entries"] / best, 1),
            "coord_updates_per_s": round(stats["coord_updates"] / best, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--full-limit", type=float, default=150.0)
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import load_movielens_npz

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev)}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    ui, iu = _pair(ds.interaction_matrix(), dev)
    _fit(ui, iu, (1.0, 1.0, 100, 500), columns=np.arange(64, dtype=np.int32))  # warm-up
    res["ml_latest_small"] = {
        "shape": list(ui.shape), "nnz": ui.nnz,
        "default": _fit(ui, iu, (1.0, 1.0, 100, None), reps=3),
        "max_nbrs_500": _fit(ui, iu, (1.0, 1.0, 100, 500), reps=3),
    }
    emit()
    del ui, iu

    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        ui, iu = _pair(ratings, dev)
        cfg = (1.0, 1.0, 100, 500)
        cols = np.sort(np.random.default_rng(20261016).choice(n_i, min(args.sample, n_i),
                                                              replace=False)).astype(np.int32)
        big = {"shape": [n_u, n_i], "nnz": int(ratings.nnz)}
        big["column_sample"] = s = _fit(ui, iu, cfg, columns=cols)
        s["sample"] = f"{len(cols)} of {n_i} columns, uniform, seeded"
        # EXTRAPOLATION: the sample's work scaled to every column at the sample's rate
        scale = n_i / len(cols)
        big["extrapolated_full_fit"] = {
            "what": "EXTRAPOLATED from the column sample, not measured",
            "resid_entries": int(s["resid_entries"] * scale),
            "coord_updates": int(s["coord_updates"] * scale),
            "seconds": round(s["seconds"] * scale, 2)}
        res["ml25m_like"] = big
        emit()
        if s["seconds"] * scale <= args.full_limit:
            big["full_fit"] = _fit(ui, iu, cfg)
            emit()
            # score + top-100 through the component, 10 000 users
            from lkpy_amd import batch as lk_batch
            from lkpy_amd.data import Dataset, Vocabulary
            from lkpy_amd.pipeline import Pipeline

            del ui, iu
            rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
            dset = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                           Vocabulary(np.arange(n_i), "item", reorder=False),
                           rows, ratings.indices, {"rating": ratings.data})
            pipe = Pipeline.load_config(ROOT / "tests" / "golden" / "pipelines" / "slim.toml")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.train(dset)
            torch.cuda.synchronize()
            t_train = time.perf_counter() - t0
            users = np.random.default_rng(43).choice(n_u, 10000, replace=False)
            lk_batch.recommend(pipe, users[:256], 100)  # uploads: training matrix, weights
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = lk_batch.recommend(pipe, users, 100)
                ts.append(time.perf_counter() - t0)
            big["recommend"] = {
                "what": "slim.toml trained through the pipeline, batch.recommend(pipe, 10 000 "
                        "user ids, 100): ids in, array-backed ItemListCollection out",
                "seconds": round(min(ts), 5), "seconds_all": [round(t, 5) for t in ts],
                "users": int(len(users)), "users_per_s": round(len(users) / min(ts), 1),
                "pipeline_train_seconds": round(t_train, 3),
                "weights": int(pipe.node("scorer").component.weights.nnz),
                "listed": int(out.total_items())}
    print(emit())


if __name__ == "__main__":
    main()
