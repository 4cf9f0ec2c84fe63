#!/usr/bin/env python3
"""``batch.score`` for ``SLIMScorer`` and ``AssociationScorer`` (mean) on the ML-25M-shaped
synthetic (``lkpy_amd.synth.ml25m_like``): 1 000 and 10 000 users x 100 sampled candidates.  Per
scorer three things are timed:

(a) the ``batch.score`` call end to end (``lk_sparse_score_candidates`` behind
    ``score_candidates_batch``), and ``batch.recommend(candidates=, n=10)``;
(b) the per-query loop ``pipe.run("scorer", query=u, items=il)`` on 200 of those users -- what the
    call did before it had a route;
(c) the composition of the kernels there were, on the same batches: per panel of at most
    ``_panel_rows()`` queries the histories cut out of the training matrix, the dense panel
    (``lk_slim_score_batch`` / ``lk_assoc_score_batch``), ``lk_panel_take_ragged`` and the
    download -- against the same steps with the new kernel in the panel's place ("route"), the
    two alternating inside one sample loop.  Their outputs are compared by bits first.

Every sample ends in a device synchronise and follows a warm-up call of the same shape; medians
with minimum and maximum of --runs samples.  Prints one JSON document, rewritten after every
scorer so that a run that is cut short leaves what it measured.  The SLIM model is fsSLIM over
``--slim-nbrs`` neighbours (the whole fit at 500 is minutes); the timings do not depend on the
models' quality, they do depend on the rows' lengths, which are reported."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_CAND, N_TOP, LOOP_USERS = 100, 10, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--slim-nbrs", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0, help="of the ML-25M shape (rehearsals)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000, 10_000])
    ap.add_argument("--scorers", nargs="+", default=["assoc-mean", "slim"])
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.data import Dataset, ItemList, Vocabulary
    from lkpy_amd.knn import AssociationScorer, SLIMScorer
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    dev = D.device()
    ratings = synth.ml25m_like(scale=args.scale)
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data})
    res = {"metric": f"seconds, ML-25M shape ({n_u} x {n_i}, {ratings.nnz} entries), "
                     f"{N_CAND} candidates per user", "device": torch.cuda.get_device_name(dev),
           "runs": args.runs, "scorers": {}}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out is not None:
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text(text + "\n")
        return text

    def stats(ts):
        return {"median": float(f"{np.median(ts):.4g}"), "min": float(f"{min(ts):.4g}"),
                "max": float(f"{max(ts):.4g}")}

    def timed(fns: dict, runs):
        "seconds per call of each function: warmed up, then ``runs`` samples each, alternating"
        for fn in fns.values():
            fn()
        torch.cuda.synchronize(dev)
        ts = {k: [] for k in fns}
        for _ in range(runs):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                ts[k].append(time.perf_counter() - t0)
        return {k: stats(v) for k, v in ts.items()}

    makers = {"slim": lambda: SLIMScorer(max_nbrs=args.slim_nbrs),
              "assoc-mean": lambda: AssociationScorer(method="lift", damping=2.0)}
    rng = np.random.default_rng(42)
    batches = {}
    for n_users in args.sizes:
        users = rng.choice(n_u, n_users, replace=False)
        items = np.stack([rng.choice(n_i, N_CAND, replace=False) for _ in range(n_users)])
        batches[n_users] = (users, items, {int(u): ItemList(items[i]) for i, u in enumerate(users)})
    first = batches[args.sizes[0]]
    loop_users = [int(u) for u in first[0][:LOOP_USERS]]

    for name in args.scorers:
        pipe = topn_pipeline(makers[name]())
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pipe.train(ds, TrainingOptions(rng=42))
        torch.cuda.synchronize(dev)
        scorer = pipe.node("scorer").component
        lookup = pipe.node("history-lookup").component
        model = scorer._device_matrix()
        lens = (model.indptr[1:] - model.indptr[:-1]).cpu().numpy()
        out = res["scorers"][name] = {
            "config": scorer.dump_config(), "train_seconds": round(time.perf_counter() - t0, 2),
            "model_entries": int(model.nnz), "model_row_median": int(np.median(lens)),
            "model_row_max": int(lens.max()), "sizes": {}}
        reduce = "sum" if name == "slim" else scorer._reduction()

        def route(users, h_ptr, nums):
            "the steps of ``batch._scored_batches`` for one batch, then the download"
            hb = lookup.batch(users)
            d_t = D.upload_targets(h_ptr, nums, dev)
            return scorer.score_candidates_batch(hb, h_ptr, nums, d_targets=d_t).cpu().numpy()

        def composition(users, h_ptr, nums):
            "the same through the dense panel, in panels of at most ``_panel_rows()`` queries"
            step = scorer._panel_rows()
            parts = []
            for lo in range(0, len(users), step):
                hi = min(len(users), lo + step)
                hb = lookup.batch(users[lo:hi])
                ptr = h_ptr[lo:hi + 1] - h_ptr[lo]
                d_ptr, d_nums = D.upload_targets(ptr, nums[h_ptr[lo]:h_ptr[hi]], dev)
                hist = hb.csr(with_values=False)
                if reduce == "sum":  # (``SLIMScorer.score_batch`` tells the empty rows itself)
                    panel = D.slim_score_batch(hist.indptr, hist.indices, model, nan_empty=True)
                else:
                    panel = D.assoc_score_batch(hist.indptr, hist.indices, model, reduce,
                                                nan_empty=True)
                parts.append(D.panel_take_ragged(panel, n_i, d_ptr, d_nums, ptr).cpu().numpy())
                del panel
            return np.concatenate(parts)

        for n_users, (users, items, cand) in batches.items():
            h_ptr = np.arange(n_users + 1, dtype=np.int64) * N_CAND
            nums = np.ascontiguousarray(items.reshape(-1), np.int32)  # (ids are numbers here)
            a, c = route(users, h_ptr, nums), composition(users, h_ptr, nums)
            same = bool(np.array_equal(a.view(np.uint32), c.view(np.uint32)))
            row = out["sizes"][str(n_users)] = {
                "route_equals_composition_by_bits": same,
                "finite": int(np.isfinite(a).sum()), "nonzero": int((a != 0).sum()),
                "history_items_median": int(np.median(lookup.batch(users).lengths)),
                "history_items_max": int(lookup.batch(users).lengths.max())}
            row.update(timed({"route": lambda: route(users, h_ptr, nums),
                              "composition": lambda: composition(users, h_ptr, nums)}, args.runs))
            row.update(timed({"score": lambda: batch.score(pipe, cand),
                              "recommend_candidates": lambda: batch.recommend(
                                  pipe, None, N_TOP, candidates=cand)}, args.runs))
            r, c_ = row["route"], row["composition"]
            row["composition_over_route"] = round(c_["median"] / r["median"], 2)
            row["spread_of_the_two"] = float(
                f"{max(r['max'] - r['min'], c_['max'] - c_['min']):.3g}")
            emit()

        def loop_score():
            for u in loop_users:
                pipe.run("scorer", query=u, items=first[2][u])

        loop = timed({"score": loop_score}, 3)["score"]
        out["per_query_loop"] = {"users": len(loop_users), **loop}
        for size, row in out["sizes"].items():
            per_user = row["score"]["median"] / int(size)
            row["score"]["loop_over_batched"] = round(
                loop["median"] / len(loop_users) / per_user, 1)
        emit()
        del pipe, scorer, model
        torch.cuda.empty_cache()
    print(emit())


if __name__ == "__main__":
    main()
