#!/usr/bin/env python3
"""``batch.predict`` through the iknn-explicit pipeline (std:topn-predict: ItemKNNScorer with the
BiasScorer fallback) at the cfg3 batch-score shape: the ML-25M-shaped synthetic,
ItemKNNScorer(max_nbrs=100, min_nbrs=1, save_nbrs=100), 10 000 users x 100 items sampled as
bench.py's batch_score leg samples them (rng 42).  Prints one JSON line: batch.predict end to end
on the DataFrame input (median of --runs, each ending in a device synchronise), the
lk_iknn_score_batch call alone on the same gathered histories, the share of the end-to-end time
outside that call, and one run of the per-query loop as the baseline (--no-loop skips it)."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.knn import ItemKNNScorer
    from lkpy_amd.pipeline import Pipeline

    dev = torch.device("cuda:0")
    ratings = synth.ml25m_like()
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data})
    pipe = Pipeline.std_topn_predict("iknn-explicit")
    pipe.replace_component("scorer", ItemKNNScorer(max_nbrs=100, min_nbrs=1, save_nbrs=100))
    pipe.train(ds)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component

    # the batch_score leg's sample (lkpy_amd/_knn_bench.py: _score_batch_leg)
    rng = np.random.default_rng(42)
    users = rng.choice(n_u, min(10_000, n_u), replace=False)
    tgt = np.sort(rng.choice(n_i, 100, replace=False)).astype(np.int32)
    df = pd.DataFrame({"user_id": np.repeat(users, len(tgt)), "item_id": np.tile(tgt, len(users))})

    def timed(fn, runs):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(min(ts))

    e2e, e2e_min = timed(lambda: batch.predict(pipe, df), args.runs)

    # the score call alone, on the histories and targets batch.predict hands it
    hb = lookup.batch(users)
    hist = hb.csr(use_ratings=True, scale=1.0, col_bias=scorer._device_means(), with_values=True)
    t_ptr = torch.from_numpy(np.arange(len(users) + 1, dtype=np.int64) * len(tgt)).to(dev)
    t_idx = torch.from_numpy(np.tile(tgt, len(users))).to(dev)
    sims = scorer._device_sims()["sims"]
    kern, kern_min = timed(lambda: D.iknn_score_batch(sims, hist.indptr, hist.indices,
                                                      hist.values, t_ptr, t_idx, 100, 1),
                           args.runs)
    res = {"metric": "batch.predict seconds, iknn-explicit (std:topn-predict), ML-25M shape, "
                     f"{len(users)} users x {len(tgt)} items, DataFrame input",
           "predict_seconds_median": round(e2e, 5), "predict_seconds_min": round(e2e_min, 5),
           "iknn_score_batch_seconds_median": round(kern, 5),
           "iknn_score_batch_seconds_min": round(kern_min, 5),
           "outside_score_call_share": round(1.0 - kern / e2e, 3), "runs": args.runs}
    if not args.no_loop:
        pairs = {int(u): np.asarray(g) for u, g in zip(users, np.split(df.item_id.to_numpy(),
                                                                      len(users)))}
        t0 = time.perf_counter()
        batch._predict_loop(pipe, pairs)
        torch.cuda.synchronize(dev)
        res["per_query_loop_seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
