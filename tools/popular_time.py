#!/usr/bin/env python3
"""
Timing driver of the Popular and Random baselines (``lkpy_amd.basic``; csrc/popular.hip).

    python tools/popular_time.py [--out profiles/popular_mi355x.json] [--sample N]

A ``PopScorer`` pipeline and a ``random_pipeline`` trained on the ML-25M-shaped synthetic of
``bench.py`` (``lkpy_amd.synth.ml25m_like``), top-100, for 10 000 users and for every user:

* ``batch.recommend`` of the Popular pipeline (the lists downloaded, as a caller gets them);
* ``lk_shared_order_topn`` alone (device events over 20 launches): the bytes it must move -- per
  row the 64-entry chunks of the order it walks (8 bytes an entry), its history row once (4 bytes
  an entry) and the list it writes (8 bytes an entry) -- over its time, beside a device copy that
  moves the same number of bytes.  The reads of the binary searches are not counted: they hit the
  row again, which the count already holds once;
* ``pipe.run`` looped over ``--sample`` users and scaled linearly to the batch: an EXTRAPOLATION;
* ``batch.recommend`` of the Random pipeline.
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


def _events(fn, launches=20, reps=3):
    "device-event seconds of ONE call: the best of ``reps`` windows of ``launches`` calls"
    import torch

    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3 / launches)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--small", action="store_true",
                    help="the synthetic at a fiftieth of the ML-25M shape (a dry run)")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import batch, synth
    from lkpy_amd.basic import PopScorer
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import random_pipeline, topn_pipeline

    dev = D.device()
    n = 100
    res = {"device": torch.cuda.get_device_name(dev), "n": n}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    mat = synth.ml25m_like(scale=0.02) if args.small else synth.ml25m_like()
    n_u, n_i = mat.shape
    rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(mat.indptr))
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False), rows, mat.indices, {})
    res["shape"] = [n_u, n_i]
    res["interactions"] = int(mat.nnz)
    res["longest_history"] = int(np.diff(mat.indptr).max())

    pop = topn_pipeline(PopScorer())
    pop.train(ds)
    rnd = random_pipeline(rng=(42, "user"))
    rnd.train(ds)
    scorer = pop.node("scorer").component
    lookup = pop.node("history-lookup").component
    some = np.sort(np.random.default_rng(20261020).choice(n_u, min(10000, n_u), replace=False))
    every = np.arange(n_u)

    for name, users in (("users_10000", some), ("users_all", every)):
        out = res[name] = {"users": int(len(users))}
        out["popular_batch_recommend"] = _timed(lambda: batch.recommend(pop, users, n))
        emit()

        # the kernel alone
        st = scorer._device_order()
        hb = lookup.batch(users)
        csr = lookup._device_matrix()["csr"]
        d_rows = torch.from_numpy(hb.user_nums).to(dev)
        idx, _ = D.shared_order_topn(st["order"], st["order_scores"], n, len(users), hist=csr,
                                     rows=d_rows)
        idx = idx.cpu().numpy()
        order = st["order"].cpu().numpy()
        where = np.zeros(n_i, np.int64)
        where[order] = np.arange(len(order))
        got = (idx >= 0).sum(axis=1)
        last = idx[np.arange(len(users)), np.maximum(got, 1) - 1]
        walked = np.where(got == n, where[np.maximum(last, 0)] + 1, len(order))
        walked = np.minimum((walked + 63) // 64 * 64, len(order))
        order_bytes = int(8 * walked.sum())
        hist_bytes = int(4 * hb.lengths.sum())
        out_bytes = int(8 * n * len(users))
        total = order_bytes + hist_bytes + out_bytes
        t = _events(lambda: D.shared_order_topn(st["order"], st["order_scores"], n, len(users),
                                                hist=csr, rows=d_rows))
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_copy = _events(lambda: dst.copy_(src))
        out["shared_order_topn_kernel"] = {
            "seconds": round(t, 7), "bytes": total, "order_bytes": order_bytes,
            "history_bytes": hist_bytes, "output_bytes": out_bytes,
            "mean_entries_walked": round(float(walked.mean()), 1),
            "GB_per_s": round(total / t / 1e9, 1),
            "device_copy_same_bytes_seconds": round(t_copy, 7),
            "device_copy_GB_per_s": round(total / t_copy / 1e9, 1)}
        del src, dst
        emit()

        out["random_batch_recommend"] = _timed(lambda: batch.recommend(rnd, users, n))
        emit()

    sample = some[:min(args.sample, len(some))]
    for name, pipe in (("popular", pop), ("random", rnd)):
        pipe.run("recommender", query=int(sample[0]), n=n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u in sample:
            pipe.run("recommender", query=int(u), n=n)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        res[f"{name}_pipe_run_loop"] = {
            "what": "pipe.run per user over a sample, EXTRAPOLATED linearly to the batches",
            "sample_users": int(len(sample)), "sample_seconds": round(t, 4),
            "extrapolated_seconds_10000": round(t * len(some) / len(sample), 2),
            "extrapolated_seconds_all": round(t * n_u / len(sample), 2)}
        emit()
    print(emit())


if __name__ == "__main__":
    main()
