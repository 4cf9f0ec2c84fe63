#!/usr/bin/env python3
"""
Timing driver of the stochastic top-N ranker (``lkpy_amd.stochastic``; csrc/stochastic.hip).

    python tools/stochastic_time.py [--out profiles/stochastic_mi355x.json] [--users N]
                                    [--sample N]

10 000 users of an ``ImplicitMFScorer`` pipeline trained on the ML-25M-shaped synthetic of
``bench.py`` (``lkpy_amd.synth.ml25m_like``), top-100:

* ``batch.recommend`` with the stochastic ranker (one sample per user) and
  ``batch.recommend_samples`` with 16 samples per user;
* beside them the deterministic ``batch.recommend`` (``TopNRanker``: the scorer's fused
  ``recommend_batch``) on the same users;
* the reference's per-list host work -- softmax, one uniform per item, the division and a top-100,
  in NumPy -- over ``--sample`` lists, scaled linearly to the batch: an EXTRAPOLATION, and a
  restatement's time, not the reference's;
* the kernels alone on one chunk of the score panel (device events): statistics pass, key pass,
  ``lk_argtopn``, with the bytes each must move and the rate against the 6.29 TB/s copy rate.
Times are host clocks around calls that end in a device synchronise unless said otherwise; warm-up
first, three repeats, the best and all three reported.  One JSON document; no threshold.
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

COPY_RATE_GBS = 6290.0


def _timed(fn, reps=3):
    import torch

    fn()  # warm-up
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return {"seconds": round(min(walls), 6), "seconds_all": [round(w, 6) for w in walls]}


def _kernel(fn, nbytes, reps=5):
    "device-event time of one call, and the rate at which it moves ``nbytes``"
    import torch

    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    gbs = nbytes / best / 1e9
    return {"seconds": round(best, 6), "bytes": int(nbytes), "GB_per_s": round(gbs, 1),
            "share_of_copy_rate": round(gbs / COPY_RATE_GBS, 4)}


def _host_loop(scores: np.ndarray, excl, n: int) -> float:
    "the reference's per-list work (_ranker.py:100-156) on the host, list by list"
    from scipy.special import softmax

    rng = np.random.default_rng(1)
    tiny = np.finfo("f4").smallest_normal
    t0 = time.perf_counter()
    for row, ex in zip(scores, excl):
        mask = np.isfinite(row)
        mask[ex] = False
        s = row[mask]
        keys = np.log(rng.uniform(0, 1, len(s))) / np.maximum(softmax(s), tiny)
        top = np.argpartition(-keys, n)[:n]
        top[np.argsort(-keys[top])]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--sample", type=int, default=2000)
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker
    from lkpy_amd.training import TrainingOptions

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "n": 100, "users": args.users}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    mat = synth.ml25m_like()
    n_u, n_i = mat.shape
    rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(mat.indptr))
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False), rows, mat.indices,
                 {"rating": mat.data})
    res["shape"] = [n_u, n_i]
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=64, epochs=2))
    pipe.train(ds, TrainingOptions(rng=42))
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    users = np.sort(np.random.default_rng(20261018).choice(n_u, args.users, replace=False))

    res["deterministic_recommend"] = _timed(lambda: batch.recommend(pipe, users, 100))
    emit()
    ranker = StochasticTopNRanker(rng=(42, "user"))
    pipe.replace_component("ranker", ranker, query="history-lookup")
    res["stochastic_recommend_1_sample"] = _timed(lambda: batch.recommend(pipe, users, 100))
    emit()
    res["stochastic_recommend_16_samples"] = _timed(
        lambda: batch.recommend_samples(pipe, users, 100, 16))
    emit()

    # the kernels alone, on one chunk of the panel
    chunk = min(len(users), batch.STOCHASTIC_PANEL_BYTES // (8 * n_i))
    hb = lookup.batch(users[:chunk])
    panel, _valid, hist = scorer.dense_scores_batch(hb)
    streams = ranker.streams(hb.user_ids)
    cells = chunk * n_i
    keys, stats = D.stochastic_keys(panel, streams, transform="softmax", scale=1.0,
                                    seed=ranker.seed, excl=hist)
    lib = D._native.require_gpu()
    res["kernels"] = {
        "rows": int(chunk),
        "row_stats": _kernel(lambda: D.check(lib.lk_stochastic_row_stats(
            D._ptr(panel), chunk, n_i, n_i, D._ptr(hist.indptr), D._ptr(hist.indices), 1, 1.0,
            D._ptr(stats), D._stream()), "lk_stochastic_row_stats"), 4 * cells),
        "keys": _kernel(lambda: D.stochastic_keys(
            panel, streams, transform="softmax", scale=1.0, seed=ranker.seed, excl=hist,
            stats=stats, out=keys), 8 * cells),
        "argtopn_100": _kernel(lambda: D.argtopn(keys, 100), 4 * cells),
    }
    emit()

    sample = min(args.sample, chunk)
    host = D.to_host(panel[:sample])
    ptr = hist.h_indptr if hist.h_indptr is not None else hist.indptr.cpu().numpy()
    idx = hist.indices.cpu().numpy()
    excl = [idx[ptr[r]:ptr[r + 1]] for r in range(sample)]
    t = _host_loop(host, excl, 100)
    res["host_loop"] = {
        "what": "per-list NumPy softmax + uniform + divide + top-100 on the host, a sample "
                "EXTRAPOLATED linearly to the batch; a restatement's time, not the reference's",
        "sample_lists": int(sample), "sample_seconds": round(t, 4),
        "extrapolated_seconds": round(t * len(users) / sample, 2)}
    print(emit())


if __name__ == "__main__":
    main()
