#!/usr/bin/env python3
"""``batch.recommend(candidates=...)`` and ``batch.score`` for ``ImplicitMFScorer`` at k = 64 on
the ML-25M-shaped synthetic (``lkpy_amd.synth.ml25m_like``): 1 000 and 10 000 users x 100 sampled
candidates, n = 10, against the per-query loop (``pipe.run("recommender", query=u, items=il,
n=10)`` / ``pipe.run("scorer", query=u, items=il)``) on 200 of those users -- the only way to get
these results without the batched calls.  Prints one JSON line: per size the median, minimum and
maximum of --runs end-to-end calls (each ending in a device synchronise, after a warm-up call of
the same shape), the seconds per user, the loop's seconds per user and the ratio; and the two new
kernels alone on the 10 000-user batch (``lk_score_candidates`` with achieved GB/s over the bytes
the scores need, ``lk_ragged_topn``; seconds per call over samples of 200 queued calls).  The
model is trained for one epoch: the timings do not depend on its quality."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_CAND, N_TOP, LOOP_USERS, K = 100, 10, 200, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, ItemList, Vocabulary
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    dev = torch.device("cuda:0")
    ratings = synth.ml25m_like()
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data})
    pipe = topn_pipeline(ImplicitMFScorer(features=K, epochs=1))
    pipe.train(ds, TrainingOptions(rng=42))
    scorer = pipe.node("scorer").component

    def timed(fn, runs, calls=1):
        "seconds per call: ``runs`` samples of ``calls`` queued calls, each ending in a synchronise"
        fn()  # warm-up at the timed shape
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / calls)
        return {"median": float(f"{np.median(ts):.4g}"), "min": float(f"{min(ts):.4g}"),
                "max": float(f"{max(ts):.4g}")}

    rng = np.random.default_rng(42)
    res = {"metric": "seconds end to end, ImplicitMFScorer k=64, ML-25M shape "
                     f"({n_u} x {n_i}), {N_CAND} candidates per user, n={N_TOP}",
           "runs": args.runs, "sizes": {}}
    loop_users = None
    for n_users in (1_000, 10_000):
        users = rng.choice(n_u, n_users, replace=False)
        items = np.stack([rng.choice(n_i, N_CAND, replace=False) for _ in range(n_users)])
        # (the collection input: what an evaluation run holds; its lists are built once, here)
        cand = {int(u): ItemList(items[i]) for i, u in enumerate(users)}
        if loop_users is None:
            loop_users = [int(u) for u in users[:LOOP_USERS]]
            loop_cand = {u: cand[u] for u in loop_users}
        res["sizes"][str(n_users)] = {
            "recommend_candidates": timed(
                lambda: batch.recommend(pipe, None, N_TOP, candidates=cand), args.runs),
            "score": timed(lambda: batch.score(pipe, cand), args.runs)}

    def loop_recommend():
        for u in loop_users:
            pipe.run("recommender", query=u, items=loop_cand[u], n=N_TOP)

    def loop_score():
        for u in loop_users:
            pipe.run("scorer", query=u, items=loop_cand[u])

    loops = {"recommend_candidates": timed(loop_recommend, 3), "score": timed(loop_score, 3)}
    res["per_query_loop"] = {"users": LOOP_USERS, **loops}
    for size, row in res["sizes"].items():
        for what in ("recommend_candidates", "score"):
            per_user = row[what]["median"] / int(size)
            loop_per_user = loops[what]["median"] / LOOP_USERS
            row[what]["seconds_per_user"] = float(f"{per_user:.3g}")
            row[what]["loop_seconds_per_user"] = float(f"{loop_per_user:.3g}")
            row[what]["loop_over_batched"] = round(loop_per_user / per_user, 1)

    # the two new kernels alone, on the 10 000-user batch
    users = rng.choice(n_u, 10_000, replace=False)
    h_ptr = np.arange(len(users) + 1, dtype=np.int64) * N_CAND
    nums = np.concatenate([rng.choice(n_i, N_CAND, replace=False) for _ in users]).astype(np.int32)
    d_ptr, d_nums = D.upload_targets(h_ptr, nums, dev)
    st = scorer._device_state()
    u = D.to_device_padded(scorer.user_embeddings[users], dev)
    rows = torch.arange(len(users), dtype=torch.int32, device=dev)
    kern = timed(lambda: D.score_candidates(u, st["Q"], K, rows, d_ptr, d_nums, h_ptr), 11, 200)
    scores = D.score_candidates(u, st["Q"], K, rows, d_ptr, d_nums, h_ptr)
    nbytes = len(nums) * (4 * K + 8)  # the item's row, its number, the score
    kern["achieved_GBps_at_median"] = round(nbytes / kern["median"] / 1e9, 1)
    res["kernels_10000_users"] = {
        "lk_score_candidates": kern,
        "lk_ragged_topn": timed(lambda: D.ragged_topn(d_ptr, d_nums, scores, N_TOP, h_ptr),
                                11, 200)}
    line = json.dumps(res)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
