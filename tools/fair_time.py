#!/usr/bin/env python3
"""
Timing driver of the FA*IR reranker (``lkpy_amd.reranking``; csrc/fair.hip).

    python tools/fair_time.py [--out profiles/fair_mi355x.json] [--sample N] [--batches N ...]

An ``ImplicitMFScorer`` pipeline (als-implicit: k = 64) trained on the ML-25M-shaped synthetic of
``bench.py`` (``lkpy_amd.synth.ml25m_like``), protected flags drawn at share 0.2, n = 100,
p = 0.5, alpha = 0.1; for 10 000 users and for all 162 541:

* ``rerank_batch`` on the scorer's own top-L lists, L = 100 and L = 400, from device tensors
  (``device_output=True``: the launch alone) and from host arrays (upload, launch, download);
* the kernel by device events, with the bytes it must move -- the row's L item numbers and L flag
  bytes read, n scores gathered, n item numbers and n scores written -- and that rate against the
  6.29 TB/s copy rate DESIGN.md quotes (an upper bound on the bytes at L = 400: the scan stops
  once both queues hold n entries);
* ``batch.recommend`` without the reranker, with it, and with ``rerank_depth=400``;
* beside each the per-list loop of ``tests/fair_restatement.py`` over ``--sample`` lists, scaled
  linearly to the batch: an EXTRAPOLATION, and a restatement's time, not the reference's.
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
sys.path.insert(0, str(ROOT / "tests"))

COPY_RATE_GBS = 6290.0
N = 100


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


def _host_loop(lists: np.ndarray, table, m, total: int) -> dict:
    import fair_restatement as R

    t0 = time.perf_counter()
    R.rerank_rows(lists, table, m, N)
    t = time.perf_counter() - t0
    return {"what": "the per-list loop of tests/fair_restatement.py on the host, a sample "
                    "EXTRAPOLATED linearly to the batch; a restatement's time, not the "
                    "reference's",
            "sample_lists": int(len(lists)), "sample_seconds": round(t, 4),
            "extrapolated_seconds": round(t * total / max(1, len(lists)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--batches", type=int, nargs="*", default=[10000, 162541])
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import Pipeline, topn_pipeline
    from lkpy_amd.reranking import FAIRReranker
    from lkpy_amd.training import TrainingOptions

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "n": N, "p": 0.5, "alpha": 0.1,
           "protected_share": 0.2, "copy_rate_GB_per_s": COPY_RATE_GBS}

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
    ds.item_attrs["protected"] = np.random.default_rng(7).random(n_i) < 0.2
    res["shape"] = [n_u, n_i]
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=64, epochs=2))
    pipe.train(ds, TrainingOptions(rng=42))
    rr = FAIRReranker(n=N)
    t0 = time.perf_counter()
    rr.train(ds)
    res["train_seconds"] = round(time.perf_counter() - t0, 3)
    res["alpha_c"] = rr.alpha_c
    both = Pipeline()
    both.nodes, both.aliases, both.default = dict(pipe.nodes), dict(pipe.aliases), pipe.default
    both.add_reranker(rr)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    flags, d_m = rr._device_tables()

    for B in args.batches:
        B = min(B, n_u)
        users = np.arange(n_u) if B == n_u else \
            np.sort(np.random.default_rng(20261018).choice(n_u, B, replace=False))
        entry = res[f"lists_{B}"] = {}
        for L in (100, 400):
            parts = [scorer.recommend_batch(lookup.batch(users[s:s + 16384]), L,
                                            device_output=True)
                     for s in range(0, B, 16384)]
            d_lists = torch.cat([p[0] for p in parts])
            d_scores = torch.cat([p[1] for p in parts])
            del parts
            h_lists, h_scores = D.to_host(d_lists), D.to_host(d_scores)
            e = entry[f"L{L}"] = {}
            e["rerank_batch_device"] = _timed(
                lambda: rr.rerank_batch(d_lists, d_scores, N, device_output=True))
            e["rerank_batch_host"] = _timed(lambda: rr.rerank_batch(h_lists, h_scores, N))
            e["kernel"] = _kernel(
                lambda: D.fair_rerank(d_lists, flags, d_m, N, scores=d_scores),
                B * (5 * L + 12 * N))
            e["kernel_without_scores"] = _kernel(
                lambda: D.fair_rerank(d_lists, flags, d_m, N), B * (5 * L + 4 * N))
            e["host_loop"] = _host_loop(h_lists[:args.sample], rr.protected_attributes,
                                        rr.m_list, B)
            del d_lists, d_scores, h_lists, h_scores
            emit()
        entry["recommend_plain"] = _timed(lambda: batch.recommend(pipe, users, N))
        entry["recommend_reranked"] = _timed(lambda: batch.recommend(both, users, N))
        emit()
        entry["recommend_plain_400"] = _timed(lambda: batch.recommend(pipe, users, 400))
        entry["recommend_rerank_depth_400"] = _timed(
            lambda: batch.recommend(both, users, N, rerank_depth=400))
        emit()
    print(emit())


if __name__ == "__main__":
    main()
