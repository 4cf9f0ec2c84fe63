#!/usr/bin/env python3
"""``batch.recommend`` and ``batch.predict`` through the als-explicit pipeline (std:topn-predict:
BiasedMFScorer with the BiasScorer fallback) at the ML-25M shape: the synthetic ratings,
``embedding_size = 64``, --users users sampled with rng 42 (default 10 000), ``n = 100``
recommendations, 20 random targets per user for the prediction.  Prints one JSON line: the two
calls end to end (after a warm-up call: the median of --runs, each ending in a device
synchronise), and -- where the scorer has the batched paths -- the kernels of one recommend panel
timed with device events (median of --runs) beside a device copy of the same panel, which is what
one read and one write of the panel cost.

The same file runs on a commit whose ``BiasedMFScorer`` has no batched path (the calls then loop
``pipe.run``): that is the baseline.  The loop is slow; give it ``--users 500 --runs 3`` and scale
linearly (the loop's cost is per query), saying so where the number is quoted."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import predict_pipeline
    from lkpy_amd.training import TrainingOptions

    dev = torch.device("cuda:0")
    ratings = synth.ml25m_like()
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data.astype(np.float32)})
    pipe = predict_pipeline(BiasedMFScorer(embedding_size=64, epochs=args.epochs))
    pipe.train(ds, TrainingOptions(rng=42))
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component

    rng = np.random.default_rng(42)
    users = rng.choice(n_u, min(args.users, n_u), replace=False)
    tgt = rng.integers(0, n_i, (len(users), 20))
    df = pd.DataFrame({"user_id": np.repeat(users, 20), "item_id": tgt.reshape(-1)})

    def timed(fn, runs):
        fn()  # warm-up
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(min(ts))

    batched = bool(getattr(scorer, "accepts_history_batch", False))
    rec, rec_min = timed(lambda: batch.recommend(pipe, users, 100), args.runs)
    pre, pre_min = timed(lambda: batch.predict(pipe, df), args.runs)
    res = {"metric": "seconds, als-explicit (std:topn-predict), ML-25M shape, k = 64, "
                     f"{len(users)} users; recommend n = 100, predict 20 targets per user",
           "batched_paths": batched, "users": int(len(users)), "runs": args.runs,
           "recommend_seconds_median": round(rec, 5), "recommend_seconds_min": round(rec_min, 5),
           "predict_seconds_median": round(pre, 5), "predict_seconds_min": round(pre_min, 5)}

    if batched:
        def events(fn, runs):
            fn()
            torch.cuda.synchronize(dev)
            ms = []
            for _ in range(runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return float(np.median(ms))

        st = scorer._device_state()
        rows = min(len(users), scorer._panel_rows())
        hb = lookup.batch(users[:rows])
        u, _mode, d_mode, ub, hist, pending = scorer._batch_operands(hb)
        for plan in pending:
            plan.check_status()
        k, g, ib = scorer.config.embedding_size, scorer.bias.global_bias, st["item_biases"]
        panel = D.score_dense(u, st["Q"], k)
        spare = torch.empty_like(panel)
        idx = D.argtopn(panel, 100)
        ms = {
            "operands (residual rows, fold-in, stored rows)": events(
                lambda: [p.check_status() for p in scorer._batch_operands(hb)[5]], args.runs),
            "lk_score_dense": events(lambda: D.score_dense(u, st["Q"], k), args.runs),
            "panel copy (device to device)": events(lambda: spare.copy_(panel), args.runs),
            "lk_bmf_finish_panel": events(
                lambda: D.bmf_finish_panel(panel, d_mode, ub, g, ib), args.runs),
            "lk_bmf_finish_panel + strike": events(
                lambda: D.bmf_finish_panel(panel, d_mode, ub, g, ib, hist.indptr, hist.indices),
                args.runs),
            "lk_argtopn": events(lambda: D.argtopn(panel, 100), args.runs),
            "lk_take_scores": events(lambda: D.take_scores(panel, idx), args.runs),
        }
        gb = 2 * panel.numel() * 4 / 1e9
        res["panel"] = {"rows": int(rows), "items": int(n_i), "read_plus_write_gb": round(gb, 3),
                        "ms": {k_: round(v, 4) for k_, v in ms.items()},
                        "finish_over_copy": round(ms["lk_bmf_finish_panel"] /
                                                  ms["panel copy (device to device)"], 3),
                        "finish_tb_per_s": round(gb / ms["lk_bmf_finish_panel"], 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
