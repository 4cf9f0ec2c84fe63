#!/usr/bin/env python3
"""
Timing driver of user-kNN's ``batch.predict`` (csrc/uknn_predict.hip) at the ML-25M shape.

    python tools/uknn_predict_time.py [--out FILE] [--users N] [--targets N] [--runs N]
                                      [--loop-users N] [--scale F] [--no-resources]

``predict_pipeline(UserKNNScorer(max_nbrs=20))`` (std:topn-predict with the BiasScorer fallback)
trained on the seeded synthetic of ``lkpy_amd.synth.ml25m_like``; --users users sampled with rng
42 (default 10 000), --targets random targets each (default 20).  One JSON document:

* ``batch.predict`` end to end: the median of --runs calls after a warm-up call, a host clock
  around calls that end in a device synchronise.
* the kernels of one step of queries (``UserKNNScorer._panel_rows`` of them) with device events,
  medians of --runs: ``lk_uknn_query_panel``, ``lk_uknn_sims_panel``, ``lk_uknn_score_pairs`` --
  beside them the query-major alternative (``lk_csr_rows_dot`` and the pairs kernel reading its
  output) -- and, in the same run, a device copy of that step's similarity panel (one read and
  one write of it), the bandwidth yardstick.  The pairs kernel's gathered bytes are counted from
  the shapes: per entry of a target's column 4 (the rater) + 4 (the rating; explicit feedback) +
  4 (the gathered similarity).
* the per-query path the batched one replaces, ``batch._predict_loop`` on the same pipeline, on
  the first --loop-users users (default 500) and SCALED linearly to --users (its cost is per
  query; the host array of all the queries' dense rows would not be reasonable to build).
* the kernel's registers, LDS and scratch as the compiler reports them
  (``-Rpass-analysis=kernel-resource-usage``).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _summary(ts):
    return {"median_s": round(statistics.median(ts), 6), "min_s": round(min(ts), 6),
            "max_s": round(max(ts), 6), "all_s": [round(t, 6) for t in ts]}


def _wall(fn, runs):
    import torch

    fn()  # warm-up
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _events(fn, runs):
    import torch

    fn()  # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
    return out


def kernel_resources():
    "what the compiler reports for the kernels of csrc/uknn_predict.hip, by template variant"
    src = ROOT / "lkpy_amd" / "csrc" / "uknn_predict.hip"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc",
           "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs",
            "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = "accumulators in LDS" if "ILb1E" in m.group(1) else "accumulators in slabs"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "uknn_predict_mi355x.json"))
    ap.add_argument("--users", type=int, default=10_000)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=500)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import pandas as pd
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native, batch, synth
    from lkpy_amd.data import Dataset, ItemList, Vocabulary
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import predict_pipeline

    _native.require_gpu()
    dev = torch.device("cuda:0")
    ratings = synth.ml25m_like() if args.scale == 1.0 else synth.ml25m_like(scale=args.scale)
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data.astype(np.float32)})
    t0 = time.perf_counter()
    pipe = predict_pipeline(UserKNNScorer(max_nbrs=20))
    pipe.train(ds)
    train_s = time.perf_counter() - t0
    print(f"trained in {train_s:.1f} s", file=sys.stderr, flush=True)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    assert batch._batched_predict_parts(pipe) is not None

    rng = np.random.default_rng(42)
    users = rng.choice(n_u, min(args.users, n_u), replace=False)
    T = args.targets
    tgt = rng.integers(0, n_i, (len(users), T))
    df = pd.DataFrame({"user_id": np.repeat(users, T), "item_id": tgt.reshape(-1)})
    res = {"device": torch.cuda.get_device_name(0),
           "metric": "seconds; predict_pipeline(UserKNNScorer(max_nbrs=20)) with the BiasScorer "
                     f"fallback, synthetic of the ML-25M shape, {len(users)} users x {T} targets",
           "shape": [int(n_u), int(n_i)], "ratings": int(ratings.nnz), "users": int(len(users)),
           "targets_per_user": T, "runs": args.runs,
           "pipeline_train_seconds": round(train_s, 3)}

    # -- batch.predict end to end ------------------------------------------------------------
    got = batch.predict(pipe, df)
    res["batch_predict"] = _summary(_wall(lambda: batch.predict(pipe, df), args.runs))
    print(f"batch.predict: {res['batch_predict']}", file=sys.stderr, flush=True)

    # -- the kernels of one step ---------------------------------------------------------------
    st, tr = scorer._device_state(), scorer._device_transposed()
    rows = min(len(users), scorer._panel_rows())
    hist = scorer._batch_csr(lookup.batch(users[:rows]))
    t_ptr = torch.arange(rows + 1, dtype=torch.int64, device=dev) * T
    t_items = torch.from_numpy(tgt[:rows].reshape(-1).astype(np.int32)).to(dev)
    thr = float(np.float32(scorer.config.min_sim))
    x = D.uknn_query_panel(hist, hist.centre)
    sims = D.uknn_sims_panel(st["vectors"], x, hist.self_user)  # [users x queries]
    sims_q = D.csr_rows_dot(st["vectors"], x)  # [queries x users]: the other layout
    spare = torch.empty_like(sims)
    out = torch.empty(rows * T, dtype=torch.float32, device=dev)

    def pairs(user_major=True):
        D.uknn_score_pairs(tr["ratings_t"], sims if user_major else sims_q, t_ptr, t_items, thr,
                           scorer.config.max_nbrs, scorer.config.min_nbrs, hist.centre,
                           self_user=hist.self_user, user_major=user_major,
                           max_col=tr["max_col"], out=out, entries=(0, rows * T))

    k = {"lk_uknn_query_panel": _summary(_events(
            lambda: D.uknn_query_panel(hist, hist.centre), args.runs)),
         "lk_uknn_sims_panel": _summary(_events(
            lambda: D.uknn_sims_panel(st["vectors"], x, hist.self_user), args.runs)),
         "lk_uknn_score_pairs": _summary(_events(pairs, args.runs)),
         "query-major instead: lk_csr_rows_dot": _summary(_events(
            lambda: D.csr_rows_dot(st["vectors"], x), args.runs)),
         "query-major instead: lk_uknn_score_pairs": _summary(_events(
            lambda: pairs(False), args.runs)),
         "similarity panel copy (device to device)": _summary(_events(
            lambda: spare.copy_(sims), args.runs))}
    col_len = np.diff(tr["ratings_t"].indptr.cpu().numpy())
    walked = int(col_len[tgt[:rows].reshape(-1)].sum())
    gathered = walked * 12
    panel_bytes = 2 * sims.numel() * 4
    pk, ck = k["lk_uknn_score_pairs"], k["similarity panel copy (device to device)"]
    res["step"] = {
        "queries": int(rows), "steps_per_call": int(-(-len(users) // rows)),
        "cells": int(rows * T), "column_entries_walked": walked,
        "longest_column": int(tr["max_col"]), "max_nbrs": int(scorer.config.max_nbrs),
        "accumulators": "LDS" if min(scorer.config.max_nbrs, tr["max_col"]) <=
        D.uknn_pairs_lds_max_nbrs() else "slabs",
        "kernels": k,
        "score_pairs_gathered_bytes": gathered,
        "score_pairs_gathered_bytes_per_s": round(gathered / pk["median_s"], 1),
        "panel_copy_bytes": panel_bytes,
        "panel_copy_bytes_per_s": round(panel_bytes / ck["median_s"], 1)}
    del x, sims, sims_q, spare
    print(f"kernels: {res['step']}", file=sys.stderr, flush=True)

    # -- the per-query path on the first --loop-users users, scaled -----------------------------
    n_loop = min(args.loop_users, len(users))
    pairs_loop = {int(u): ItemList(item_ids=tgt[r]) for r, u in enumerate(users[:n_loop])}
    first = dict(list(pairs_loop.items())[:8])
    batch._predict_loop(pipe, first)  # warm-up: the device copies of the model
    ts = []
    for _ in range(min(args.runs, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = batch._predict_loop(pipe, pairs_loop)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        print(f"per-query loop, {n_loop} users: {ts[-1]:.2f} s", file=sys.stderr, flush=True)
        if ts[-1] > 60.0:
            break  # (slow enough that one repeat says it)
    loop = _summary(ts)
    scale = len(users) / n_loop
    res["per_query_loop"] = {"users": int(n_loop), **loop, "scaled_to_users": int(len(users)),
                             "scaled_median_s": round(loop["median_s"] * scale, 4)}
    res["batched_over_scaled_loop"] = round(
        res["batch_predict"]["median_s"] / (loop["median_s"] * scale), 5)
    # the two paths answer alike (the timed calls' own results)
    same = True
    for u, w in want:
        g = got.lookup(u.user_id)
        a, b = np.asarray(g.scores(), np.float32), np.asarray(w.scores(), np.float32)
        same = same and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
            a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    res["loop_users_bit_equal"] = bool(same)

    if not args.no_resources:
        res["kernel_resource_usage"] = kernel_resources()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k_: v for k_, v in res.items() if k_ != "step"}))


if __name__ == "__main__":
    main()
