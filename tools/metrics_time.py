#!/usr/bin/env python3
"""
Timing driver of run evaluation (``lkpy_amd.metrics``; csrc/metrics.hip) on the device.

    python tools/metrics_time.py [--out FILE] [--no-ml25m] [--sample N]

* ml-latest-small (tests/golden/ml_small.npz): ``measure_run`` of the ``quick_measure_model``
  metric set on the 134 x 20 lists of an ``ImplicitMFScorer`` pipeline.
* the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``), a seeded 20 % of
  every user's row held out: the truth upload (once), then ``measure_run`` for 10 000 x 100 and
  162 541 x 100 lists, from host arrays and from device tensors, split into key matching /
  gather / kernels / download / host composition (the split run synchronises between the parts);
  next to it ``batch.recommend`` for the same 10 000 users, so the evaluation's share of
  recommend + evaluate is a measured ratio.
* the yardstick for what this replaces: the per-list loop of ``tests/metrics_restatement.py``
  over ``--sample`` lists on this machine's host, scaled linearly to the batch -- an
  EXTRAPOLATION, and a restatement's time, not the reference's.
Times are host clocks around calls that end in a device synchronise; warm-up first, three
repeats, the best and all three reported.  One JSON document.
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


def _quick_set():
    from lkpy_amd import metrics as M

    mc = M.MeasurementCollector()
    for m in (M.RecipRank(), M.RBP(), M.NDCG(), M.Hit(), M.Recall()):
        mc.add_metric(m)
    return mc


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


def _measure(mc, keys, nums, test, vocab):
    "one measure_run from arrays (host or device); returns the run and the split of its time"
    def run():
        c = mc.empty_copy()
        c.add_array_measurements(keys, nums, test, vocabulary=vocab)
        return c.summary_metrics(), c.list_metrics()

    out = _timed(run)
    split = {}
    c = mc.empty_copy()
    c.add_array_measurements(keys, nums, test, vocabulary=vocab, timing=split)
    out["split_s"] = {k: round(v, 6) for k, v in split.items()}
    out["lists"] = int(len(keys))
    return out


def _restatement_loop(lists, truth_of, sample):
    "the per-list loop over ``sample`` lists: the five quick metrics per list"
    import metrics_restatement as R

    t0 = time.perf_counter()
    for q in sample:
        recs = lists[q][lists[q] >= 0]
        t = truth_of(q)
        R.recip_rank(recs, t), R.rbp(recs, t), R.ndcg(recs, t), R.hit(recs, t), R.recall(recs, t)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--sample", type=int, default=2000)
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch
    from lkpy_amd import metrics as M
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, ItemListCollection, Vocabulary, load_movielens_npz
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.splitting import SampleFrac, sample_users
    from lkpy_amd.training import TrainingOptions

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev)}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    split = sample_users(ds, 134, SampleFrac(0.2, rng=42), rng=42)
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=50, epochs=10))
    pipe.train(split.train, TrainingOptions(rng=42))
    users = np.asarray(split.test._lists.raw_keys)
    recs = batch.recommend(pipe, users, 20)
    mc = _quick_set()
    small = _timed(lambda: mc.measure_run(recs, split.test))
    run = mc.measure_run(recs, split.test)
    small["lists"] = len(recs)
    small["summary"] = {k: v for k, v in run.summary_metrics.items() if k.endswith(".mean")}
    nums = recs._lists.nums
    ids = split.train.items.ids()
    tl = split.test._lists
    t = _restatement_loop(np.where(nums >= 0, ids[np.maximum(nums, 0)], -1),
                          lambda q: tl.item_ids[tl.offsets[q]:tl.offsets[q + 1]],
                          range(len(users)))
    small["restatement_loop_seconds"] = round(t, 6)
    res["ml_latest_small"] = small
    emit()

    if not args.no_ml25m:
        from lkpy_amd import synth

        mat = synth.ml25m_like()
        n_u, n_i = mat.shape
        rng = np.random.default_rng(20261016)
        indptr = mat.indptr.astype(np.int64)
        lens = np.diff(indptr)
        rows = np.repeat(np.arange(n_u, dtype=np.int32), lens)
        order = np.argsort(rows + rng.random(mat.nnz), kind="stable")
        p = np.arange(mat.nnz) - np.repeat(indptr[:-1], lens)
        held = np.zeros(mat.nnz, bool)
        held[order[p < np.repeat(np.round(lens * 0.2).astype(np.int64), lens)]] = True
        offsets = np.zeros(n_u + 1, np.int64)
        np.cumsum(np.bincount(rows[held], minlength=n_u), out=offsets[1:])
        t_items = mat.indices[held].astype(np.int64)
        keys = np.arange(n_u, dtype=np.int64)
        test = ItemListCollection.from_ragged(keys, offsets, t_items,
                                              {"rating": mat.data[held].astype(np.float32)})
        train = Dataset(Vocabulary(keys, "user", reorder=False),
                        Vocabulary(np.arange(n_i), "item", reorder=False), rows[~held],
                        mat.indices[~held], {"rating": mat.data[~held]})
        big = {"shape": [n_u, n_i], "nnz": int(mat.nnz), "test_pairs": int(held.sum())}
        pipe = topn_pipeline(ImplicitMFScorer(embedding_size=64, epochs=2))
        pipe.train(train, TrainingOptions(rng=42))
        scorer = pipe.node("scorer").component
        lookup = pipe.node("history-lookup").component
        some = np.sort(rng.choice(n_u, 10000, replace=False))
        big["recommend_10000x100"] = _timed(lambda: batch.recommend(pipe, some, 100))

        def device_lists(us):
            parts = [scorer.recommend_batch(lookup.batch(us[s:s + 16384]), 100,
                                            device_output=True)[0]
                     for s in range(0, len(us), 16384)]
            return parts[0] if len(parts) == 1 else torch.cat(parts)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts = M.truth_state(test, scorer.items)
        ts.device_csr(None, dev)
        torch.cuda.synchronize()
        big["truth_build_and_upload_seconds"] = round(time.perf_counter() - t0, 6)
        for name, us in (("10000x100", some), ("162541x100", keys)):
            d_nums = device_lists(us)
            h_nums = D.to_host(d_nums)
            big[f"measure_run_{name}_host_arrays"] = _measure(mc, us, h_nums, test, scorer.items)
            big[f"measure_run_{name}_device_tensors"] = _measure(mc, us, d_nums, test,
                                                                 scorer.items)
            sample = rng.choice(len(us), min(args.sample, len(us)), replace=False)
            t = _restatement_loop(h_nums, lambda q, us=us: t_items[offsets[us[q]]:
                                                                   offsets[us[q] + 1]], sample)
            big[f"restatement_loop_{name}"] = {
                "what": "per-list NumPy restatement on the host, a sample EXTRAPOLATED linearly "
                        "to the batch; a restatement's time, not the reference's",
                "sample_lists": int(len(sample)), "sample_seconds": round(t, 4),
                "extrapolated_seconds": round(t * len(us) / len(sample), 2)}
            del d_nums, h_nums
            res["ml25m_like"] = big
            emit()
        rec = big["recommend_10000x100"]["seconds"]
        ev = big["measure_run_10000x100_host_arrays"]["seconds"]
        big["evaluate_share_of_recommend_plus_evaluate_10000"] = round(ev / (ev + rec), 4)
    print(emit())


if __name__ == "__main__":
    main()
