#!/usr/bin/env python3
"""
Timing driver of user-kNN's ``batch.recommend`` (csrc/uknn_recommend.hip) on the device.

    python tools/uknn_time.py [--out FILE] [--users N] [--scale F] [--no-synth]
                              [--loop-users N] [--loop-limit SECONDS] [--commit TEXT]

* ``batch.recommend(topn_pipeline(UserKNNScorer(k=30)), users, 100)`` on ml-latest-small
  (tests/golden/ml_small.npz, every user) and on the ML-25M-shaped synthetic of
  ``lkpy_amd.synth.ml25m_like(scale=--scale)`` (``--users`` users): medians of repeated calls
  after a warm-up, every repeat listed, and the time per 1 000 users.  On a tree whose scorer has no
  ``recommend_batch`` the same call runs the pipeline once per user: it is then given at most
  ``--loop-users`` users or ``--loop-limit`` seconds per repeat, and the figure per 1 000 users is
  EXTRAPOLATED from the users done (and named so).
* where the panel kernels exist: the three of them (``lk_uknn_query_panel``,
  ``lk_uknn_sims_panel``, ``lk_uknn_score_panel``) and ``lk_argtopn`` + ``lk_take_scores``
  separately for one panel of the batch, and the score kernel's bytes -- per (item, block of 64
  queries) 8 per column entry + 256 per similarity row read, + 4 per panel cell -- over its time
  next to a measured device copy rate.
Times are device events around the kernels, host clocks around calls that end in a device
synchronise.  One JSON document.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _summary(ts):
    return {"median_s": round(statistics.median(ts), 6), "min_s": round(min(ts), 6),
            "max_s": round(max(ts), 6), "all_s": [round(t, 6) for t in ts]}


def _wall(fn, reps):
    import torch

    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _events(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def copy_rate(dev):
    "bytes/s (read + write) of a device-to-device copy of 2 GiB"
    import torch

    a = torch.empty(1 << 29, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    ts = [_events(lambda: b.copy_(a)) for _ in range(5)]
    return round(2 * a.numel() * 4 / statistics.median(ts), 1), _summary(ts)


def kernel_legs(scorer, lookup, users, n, reps):
    "the three panel kernels and the selection, separately, for the first panel of the batch"
    from lkpy_amd import _device as D

    hist = scorer._batch_csr(lookup.batch(users))
    hi = min(hist.shape[0], scorer._panel_rows())
    st, tr = scorer._device_state(), scorer._device_transposed()
    rt = tr["ratings_t"]
    thr = float(np.float32(scorer.config.min_sim))
    cfg = scorer.config
    box = {}
    legs = {
        "query_panel": lambda: box.update(
            x=D.uknn_query_panel(hist, hist.centre, rows=(0, hi))),
        "sims_panel": lambda: box.update(
            sims=D.uknn_sims_panel(st["vectors"], box["x"], hist.self_user[:hi])),
        "score_panel": lambda: box.update(panel=D.uknn_score_panel(
            rt, box["sims"], hi, thr, cfg.max_nbrs, cfg.min_nbrs,
            None if hist.centre is None else hist.centre[:hi], hist=hist, rows=(0, hi),
            strike_history=True, item_order=tr["order"], max_col=tr["max_col"])),
        "argtopn+take_scores": lambda: D.take_scores(box["panel"], D.argtopn(box["panel"], n)),
    }
    times = {k: [] for k in legs}
    for rep in range(reps + 1):
        for k, fn in legs.items():
            t = _events(fn)
            if rep:  # (the first pass is the warm-up)
                times[k].append(t)
    n_items, n_users = rt.shape
    blocks = (hi + 63) // 64
    n_bytes = blocks * (8 + 256) * rt.nnz + 4 * hi * n_items
    out = {"panel_queries": int(hi), "panel_rows_limit": int(scorer._panel_rows()),
           "users": int(n_users), "items": int(n_items), "ratings": int(rt.nnz),
           "longest_column": int(tr["max_col"]), "max_nbrs": int(cfg.max_nbrs),
           "accumulators": "LDS" if min(cfg.max_nbrs, tr["max_col"]) <= D.uknn_lds_max_nbrs()
           else "global slab",
           "score_panel_bytes": int(n_bytes)}
    for k, ts in times.items():
        out[k] = _summary(ts)
    out["score_panel"]["bytes_per_s"] = round(n_bytes / out["score_panel"]["median_s"], 1)
    return out


def recommend_legs(ds, users, n, reps, loop_users, loop_limit):
    from lkpy_amd import batch
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import topn_pipeline

    scorer = UserKNNScorer(k=30, min_sim=1.0e-6)
    pipe = topn_pipeline(scorer)
    t_train = _wall(lambda: pipe.train(ds), 1)[0]
    lookup = pipe.node("history-lookup").component
    out = {"pipeline_train_seconds": round(t_train, 4), "n": n,
           "shape": [int(ds.user_count), int(ds.item_count)]}
    if hasattr(scorer, "recommend_batch"):
        batch.recommend(pipe, users[:64], n)  # warm-up: uploads, the transpose, the centres
        out["path"] = "recommend_batch: whole panels on the device"
        out["users"] = int(len(users))
        out["recommend"] = r = _summary(_wall(lambda: batch.recommend(pipe, users, n), reps))
        per_user = [t / len(users) for t in r["all_s"]]
        out["kernels"] = kernel_legs(scorer, lookup, users, n, reps)
    else:
        out["path"] = "one pipe.run per user (no recommend_batch); per 1 000 users EXTRAPOLATED " \
                      "from the users done"
        batch.recommend(pipe, users[:2], n)  # warm-up
        per_user, done_all, ts = [], [], []
        for _ in range(reps):
            import torch

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = 0
            for u in np.asarray(users[:loop_users]).tolist():
                batch.recommend(pipe, [u], n)
                done += 1
                if time.perf_counter() - t0 > loop_limit:
                    break
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            done_all.append(done)
            per_user.append(ts[-1] / done)
        out["users"] = done_all
        out["recommend"] = _summary(ts)
    out["seconds_per_1000_users"] = {
        "median": round(1000 * statistics.median(per_user), 4),
        "min": round(1000 * min(per_user), 4), "max": round(1000 * max(per_user), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--no-synth", action="store_true")
    ap.add_argument("--loop-users", type=int, default=64)
    ap.add_argument("--loop-limit", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="what the capture was taken from")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "capture_commit": args.commit}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    rate, spread = copy_rate(dev)
    res["device_copy"] = {"bytes_per_s": rate, **spread}
    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    res["ml_latest_small"] = recommend_legs(ds, ds.users.ids(), 100, args.reps, args.loop_users,
                                            args.loop_limit)
    emit()
    if not args.no_synth:
        from lkpy_amd import synth

        ratings = synth.ml25m_like(scale=args.scale)
        n_u, n_i = ratings.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        dset = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                       Vocabulary(np.arange(n_i), "item", reorder=False),
                       rows, ratings.indices, {"rating": ratings.data})
        users = np.random.default_rng(43).choice(n_u, min(args.users, n_u), replace=False)
        res[f"ml25m_like_scale_{args.scale:g}"] = recommend_legs(
            dset, users, 100, max(2, args.reps - 2), args.loop_users, args.loop_limit)
    print(emit())


if __name__ == "__main__":
    main()
