#!/usr/bin/env python3
"""
Timing driver of the exposure / diversity / popularity / reranking metrics
(``lkpy_amd.metrics``, ``lkpy_amd.reranking_metrics``; csrc/diversity.hip) on the device.

    python tools/diversity_time.py [--out FILE] [--sample N] [--small-only]

Synthetic top-100 lists over 62 423 items (the ML-25M item count; distinct items per list, a
heavy head: the most popular item sits in about 1 % of the lists), 10 000 and 162 541 of them,
as device tensors.  Per size, ``add_array_measurements`` + ``summary_metrics`` of each metric
group and of the full set:

* ``gini``: ListGini + ExposureGini@100;
* ``genres``: ILS + Entropy + RankBiasedEntropy over a sparse 62 423 x 20 matrix (about 2.4
  genres per item); ``tags``: the same three over a DENSE 62 423 x 1128 matrix;
* ``pop``: MeanPopRank;
* ``rbo_lip_n10``: rank_biased_overlap_collection + least_item_promoted_collection (n = 10) of
  reshuffled samples of every list against the list itself: four samples per list at 10 000
  lists (40 000 pairs), one per list at 162 541 (the time is the host's: packing both
  collections into ragged arrays; four samples there would only multiply it).  The two
  compare TWO collections and are no collector metrics, so they are timed beside the ``all`` set,
  not inside it.

Next to each figure the per-list loop of ``tests/diversity_restatement.py`` over ``--sample``
lists on this machine's host, scaled linearly to the batch -- an EXTRAPOLATION, and a
restatement's time, not the reference's.  Times are host clocks around calls that end in a device
synchronise; warm-up first, three repeats, the best and all three reported.  One JSON document.
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

N_ITEMS = 62423


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


def _lists(rng, B, n=100):
    "B lists of n distinct items, popular (low-numbered) items far more often, in random order"
    pos = np.cumsum(rng.geometric(0.01, (B, n)), axis=1) - 1
    assert pos.max() < N_ITEMS
    return rng.permuted(pos, axis=1).astype(np.int32)


def _loop(fn, lists, sample, B):
    t0 = time.perf_counter()
    for q in sample:
        fn(lists[q])
    t = time.perf_counter() - t0
    return {"sample_lists": int(len(sample)), "sample_seconds": round(t, 4),
            "extrapolated_seconds": round(t * B / len(sample), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--small-only", action="store_true")
    args = ap.parse_args()

    import diversity_restatement as R
    import scipy.sparse as sps
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import metrics as M
    from lkpy_amd import reranking_metrics as RM
    from lkpy_amd.data import Dataset, ItemList, ItemListCollection, Vocabulary

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "n_items": N_ITEMS,
           "restatement_note": "per-list NumPy restatement on the host, a sample EXTRAPOLATED "
                               "linearly to the batch; a restatement's time, not the reference's"}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    rng = np.random.default_rng(20261018)
    vocab = Vocabulary(np.arange(N_ITEMS), "item", reorder=False)
    genres = sps.csr_array((rng.random((N_ITEMS, 20)) < 0.12).astype(np.float64))
    tags = rng.random((N_ITEMS, 1128))
    n_int = 2_000_000
    ds = Dataset(Vocabulary(np.arange(5000), "user", reorder=False), vocab,
                 rng.integers(0, 5000, n_int),
                 np.minimum(rng.geometric(0.0005, n_int) - 1, N_ITEMS - 1), {})
    test = ItemListCollection.from_dict({0: ItemList(item_ids=[0])}, key=("user_id",))
    geo = M.GeometricRankWeight(0.85)
    groups = {
        "gini": [M.ListGini(items=vocab), M.ExposureGini(100, items=vocab)],
        "genres_c20_sparse": [M.ILS(categories=genres, items=vocab, attribute="genre"),
                              M.Entropy(categories=genres, items=vocab, attribute="genre"),
                              M.RankBiasedEntropy(categories=genres, items=vocab,
                                                  attribute="genre", weight=geo)],
        "tags_c1128_dense": [M.ILS(categories=tags, items=vocab, attribute="tag"),
                             M.Entropy(categories=tags, items=vocab, attribute="tag"),
                             M.RankBiasedEntropy(categories=tags, items=vocab, attribute="tag",
                                                 weight=geo)],
        "pop": [M.MeanPopRank(ds)],
    }
    groups["all"] = [m for ms in groups.values() for m in ms]
    g_unit, g_dist = (R.normalize_rows(genres.toarray(), k) for k in ("unit", "distribution"))
    t_unit, t_dist = (R.normalize_rows(tags, k) for k in ("unit", "distribution"))
    table = groups["pop"][0].item_ranks

    def cat_loop(unit, dist):
        return lambda r: (R.ils(r, unit), R.entropy(r, dist),
                          R.entropy(r, dist, None, R.geometric_weight))

    loops = {
        "gini": None,  # (timed over the sample as ONE accumulation, see below)
        "genres_c20_sparse": cat_loop(g_unit, g_dist),
        "tags_c1128_dense": cat_loop(t_unit, t_dist),
        "pop": lambda r: R.mean_pop_rank(r, table),
    }

    for B in (10000,) if args.small_only else (10000, 162541):
        h_lists = _lists(rng, B)
        d_lists = torch.from_numpy(h_lists).to(dev)
        keys = np.arange(B, dtype=np.int64)
        sample = rng.choice(B, min(args.sample, B), replace=False)
        out = {}
        for name, ms in groups.items():
            mc = M.MeasurementCollector()
            for m in ms:
                mc.add_metric(m)

            def run(nums, mc=mc):
                c = mc.empty_copy()
                c.add_array_measurements(keys, nums, test, vocabulary=vocab)
                return c.summary_metrics()

            entry = {"device_tensors": _timed(lambda: run(d_lists))}
            if name == "all":
                entry["host_arrays"] = _timed(lambda: run(h_lists))
            elif name == "gini":
                t0 = time.perf_counter()
                R.gini_of_totals(R.exposure_totals([h_lists[q] for q in sample], N_ITEMS))
                R.gini_of_totals(R.exposure_totals([h_lists[q] for q in sample], N_ITEMS, 100,
                                                   R.geometric_weight))
                t = time.perf_counter() - t0
                entry["restatement_loop"] = {
                    "sample_lists": int(len(sample)), "sample_seconds": round(t, 4),
                    "extrapolated_seconds": round(t * B / len(sample), 2)}
            else:
                entry["restatement_loop"] = _loop(loops[name], h_lists, sample, B)
            out[name] = entry
            res[f"lists_{B}x100"] = out
            emit()
        n_samples = 4 if B == 10000 else 1  # reshuffled samples per list against the list itself
        ref = ItemListCollection.from_arrays(keys, h_lists, np.zeros(h_lists.shape, np.float32),
                                             vocab, key=("user_id",))
        s_lists = rng.permuted(np.repeat(h_lists, n_samples, axis=0), axis=1)
        pairs = np.stack([np.repeat(keys, n_samples), np.tile(np.arange(n_samples), B)], axis=1)
        rer = ItemListCollection.from_arrays(pairs, s_lists, np.zeros(s_lists.shape, np.float32),
                                             vocab, key=("user_id", "sample"))
        entry = {"pairs": len(pairs), "device": _timed(lambda: (
            RM.rank_biased_overlap_collection(ref, rer),
            RM.least_item_promoted_collection(ref, rer)))}
        entry["restatement_loop"] = _loop(
            lambda q: (R.rbo(h_lists[q // n_samples], s_lists[q]),
                       R.lip(h_lists[q // n_samples], s_lists[q])),
            np.arange(len(pairs)), rng.choice(len(pairs), min(args.sample, len(pairs)),
                                              replace=False), len(pairs))
        out["rbo_lip_n10"] = entry
        emit()
        del d_lists
    print(emit())


if __name__ == "__main__":
    main()
