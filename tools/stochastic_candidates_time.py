#!/usr/bin/env python3
"""Sampled and random rankings of per-user candidate lists on the ML-25M-shaped synthetic (``lkpy_amd.synth.ml25m_like``): 1 000 and
10 000 users x 100 sampled candidates, n = 10, k = 64.  Timed end to end (each call ends in a
device synchronise, after a warm-up call of the same shape; median, minimum and maximum of --runs):

- ``batch.recommend(candidates=)`` with a ``StochasticTopNRanker`` over ``ImplicitMFScorer``;
- ``batch.recommend_samples(candidates=)`` with 16 samples;
- ``batch.recommend(candidates=)`` of a ``random_pipeline``;

each against the per-query loop -- ``pipe.run`` user by user, the only path before these routes
existed -- on 500 of the users, scaled per user.  And the key kernel against the dense detour:
``stochastic.rank_ragged`` on the scored lists against a scatter of the same scores into a
[rows x items] NaN panel followed by ``stochastic.rank_panel`` (in chunks of 2 000 rows), whose
lists are compared before anything is timed.  Prints one JSON line; ``--out`` also writes it.  The
models are trained for one epoch: the timings do not depend on their quality."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_CAND, N_TOP, LOOP_USERS, K, SAMPLES, PANEL_ROWS = 100, 10, 500, 64, 16, 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from lkpy_amd import batch, synth
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, ItemList, Vocabulary
    from lkpy_amd.pipeline import random_pipeline, topn_pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker, rank_panel, rank_ragged
    from lkpy_amd.training import TrainingOptions

    dev = torch.device("cuda:0")
    ratings = synth.ml25m_like()
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data})
    sto = topn_pipeline(ImplicitMFScorer(features=K, epochs=1))
    sto.train(ds, TrainingOptions(rng=42))
    sto.replace_component("ranker", StochasticTopNRanker(rng=(7, "user")), query="history-lookup")
    ranker = sto.node("ranker").component
    rnd = random_pipeline(rng=(7, "user"))
    rnd.train(ds)

    def timed(fn, runs):
        fn()  # warm-up at the timed shape
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return {"median": float(f"{np.median(ts):.4g}"), "min": float(f"{min(ts):.4g}"),
                "max": float(f"{max(ts):.4g}")}

    rng = np.random.default_rng(42)
    res = {"metric": f"seconds end to end, k={K}, ML-25M shape ({n_u} x {n_i}), {N_CAND} "
                     f"candidates per user, n={N_TOP}, {SAMPLES} samples in recommend_samples",
           "runs": args.runs, "sizes": {}, "keys_vs_dense": {}}
    calls = {
        "stochastic_recommend": lambda c: batch.recommend(sto, None, N_TOP, candidates=c),
        "stochastic_samples": lambda c: batch.recommend_samples(sto, None, N_TOP, SAMPLES,
                                                                candidates=c),
        "random_recommend": lambda c: batch.recommend(rnd, None, N_TOP, candidates=c),
    }
    loop_cand = None
    for n_users in (1_000, 10_000):
        users = rng.choice(n_u, n_users, replace=False)
        items = np.stack([rng.choice(n_i, N_CAND, replace=False) for _ in range(n_users)])
        cand = {int(u): ItemList(items[i]) for i, u in enumerate(users)}
        if loop_cand is None:
            loop_cand = {int(u): cand[int(u)] for u in users[:LOOP_USERS]}
        res["sizes"][str(n_users)] = {
            what: timed(lambda: fn(cand), args.runs) for what, fn in calls.items()}

        # the key kernel against the dense detour, on this batch's scored lists
        h_ptr = np.arange(n_users + 1, dtype=np.int64) * N_CAND
        d_scores = torch.randn(n_users * N_CAND, dtype=torch.float32, device=dev)
        streams = ranker.streams(users)
        opts = dict(transform="softmax", scale=1.0, seed=ranker.seed)
        # the panel a per-query call would form is [1 x 100]; the DETOUR of a batch by item
        # number is [rows x items], which is what is timed here -- so address by number too
        order = np.argsort(items, axis=1, kind="stable")
        by_num = np.take_along_axis(items, order, axis=1).reshape(-1).astype(np.int32)
        d_sorted = d_scores.view(n_users, N_CAND)[
            torch.arange(n_users, device=dev)[:, None], torch.from_numpy(order).to(dev)
        ].reshape(-1).contiguous()
        wide = np.full(n_users, n_i, np.int32)

        def ragged():
            return rank_ragged(h_ptr, by_num, None, d_sorted, wide, streams, N_TOP,
                               device_output=True, **opts)

        d_rows = torch.arange(n_users, device=dev).repeat_interleave(N_CAND)
        d_cols = torch.from_numpy(by_num.astype(np.int64)).to(dev)

        def dense():
            out = []
            for lo in range(0, n_users, PANEL_ROWS):
                hi = min(n_users, lo + PANEL_ROWS)
                panel = torch.full((hi - lo, n_i), float("nan"), dtype=torch.float32, device=dev)
                sel = slice(lo * N_CAND, hi * N_CAND)
                panel[d_rows[sel] - lo, d_cols[sel]] = d_sorted[sel]
                out.append(rank_panel(panel, streams[lo:hi], N_TOP, device_output=True, **opts))
            return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

        (ri, rk), (di, dk) = ragged(), dense()
        same = bool(torch.equal(ri, di) and torch.equal(rk.view(torch.int32),
                                                         dk.view(torch.int32)))
        res["keys_vs_dense"][str(n_users)] = {
            "same_lists_and_key_bits": same, "rank_ragged": timed(ragged, args.runs),
            "scatter_and_rank_panel": timed(dense, args.runs)}

    def loop(pipe, node, **kw):
        return lambda: [pipe.run(node, query=u, items=il, **kw) for u, il in loop_cand.items()]

    def loop_samples():
        for u, il in loop_cand.items():
            got = sto.run_all("history-lookup", "scorer", query=u, items=il)
            ranker.sample(got["scorer"], got["history-lookup"], N_TOP, samples=SAMPLES)

    loops = {"stochastic_recommend": timed(loop(sto, "recommender", n=N_TOP), 3),
             "stochastic_samples": timed(loop_samples, 3),
             "random_recommend": timed(loop(rnd, "recommender", n=N_TOP), 3)}
    res["per_query_loop"] = {"users": LOOP_USERS, **loops}
    for size, row in res["sizes"].items():
        for what in calls:
            per_user = row[what]["median"] / int(size)
            loop_per_user = loops[what]["median"] / LOOP_USERS
            row[what]["seconds_per_user"] = float(f"{per_user:.3g}")
            row[what]["loop_seconds_per_user"] = float(f"{loop_per_user:.3g}")
            row[what]["loop_over_batched"] = round(loop_per_user / per_user, 1)
    for row in res["keys_vs_dense"].values():
        row["dense_over_ragged"] = round(row["scatter_and_rank_panel"]["median"] /
                                         row["rank_ragged"]["median"], 1)
    line = json.dumps(res)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
