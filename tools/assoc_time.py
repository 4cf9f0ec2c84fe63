#!/usr/bin/env python3
"""
Timing driver of the association-rule trainer and scorer (csrc/assoc.hip) on the device.

    python tools/assoc_time.py [--out FILE] [--no-ml25m] [--users N] [--host-lists N]
                               [--host-limit SECONDS] [--commit TEXT]

* training, split into the co-occurrence build (``iknn_build`` on unit values), the scaling
  (``lk_assoc_scale``) and the download, on ml-latest-small (tests/golden/ml_small.npz) and on the
  ML-25M-shaped synthetic of ``lkpy_amd.synth.ml25m_like``: medians of repeated calls after a
  warm-up, every repeat listed;
* ``recommend_batch`` for ``--users`` users, top-100, mean and max (``biased-lift.toml`` trained
  through the pipeline);
* the scoring kernel alone against the baseline it has to meet: ``lk_slim_score_batch`` on the same
  CSR and the same histories forms the same sums (one workgroup per query, accumulator row in
  global memory, a barrier per history item).  The two are timed alternately, with and without
  ``lk_argtopn`` behind them; the kernel's bytes (8 per stored entry of every reference row + 4 per
  panel cell) over its time stand next to a measured device copy rate.  The mean panel is checked
  against the baseline's sums divided in float64 (the same bits);
* the per-query host loop (densify the reference rows, ``np.mean``, strike, top-100) on the same
  machine, over at most ``--host-lists`` lists or ``--host-limit`` seconds, extrapolated (and named
  so) to the batch.
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


def _binary_pair(ratings, dev):
    import scipy.sparse as sps

    from lkpy_amd import _device as D

    ui = sps.csr_array(ratings).astype(np.float32)
    ui.sum_duplicates()
    ui.data[:] = 1.0
    ui.sort_indices()
    iu = sps.csr_array(ui.T)
    iu.sort_indices()
    return D.DeviceCSR.from_scipy(ui, dev), D.DeviceCSR.from_scipy(iu, dev), \
        np.diff(iu.indptr).astype(np.int32)


def train_split(ratings, dev, reps):
    "build / scale / download of one fit (lift, damping 20), ``reps`` times after a warm-up"
    import torch

    from lkpy_amd import _device as D

    ui, iu, counts = _binary_pair(ratings, dev)
    d_counts = torch.from_numpy(counts).to(dev)
    n_groups, n_items = ui.shape
    legs = {"build": [], "scale": [], "download": []}
    nnz = 0
    for rep in range(reps + 1):
        box = {}
        t_build = _wall(lambda: box.update(c=D.iknn_build(ui, iu, 0.5)), 1)[0]
        cooc = box.pop("c")
        t_scale = _wall(lambda: D.assoc_scale(cooc, d_counts, n_groups, "lift", 20.0), 1)[0]
        t_down = _wall(lambda: (D.to_host(cooc.values),
                                D.to_host(cooc.indices, index_bound=n_items),
                                cooc.indptr.cpu()), 1)[0]
        nnz = cooc.nnz
        del cooc
        if rep:  # (the first pass is the warm-up)
            legs["build"].append(t_build)
            legs["scale"].append(t_scale)
            legs["download"].append(t_down)
    out = {"shape": [int(n_groups), int(n_items)], "interactions": int(ui.nnz),
           "stored_pairs": int(nnz), "config": {"method": "lift", "damping": 20.0}}
    out.update({k: _summary(v) for k, v in legs.items()})
    out["scale"]["bytes_per_s"] = round(12 * nnz / out["scale"]["median_s"], 1)  # idx + val in/out
    return out


def copy_rate(dev):
    "bytes/s (read + write) of a device-to-device copy of 2 GiB"
    import torch

    a = torch.empty(1 << 29, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    ts = [_events(lambda: b.copy_(a)) for _ in range(5)]
    return round(2 * a.numel() * 4 / statistics.median(ts), 1), _summary(ts)


def score_legs(scorer, hist, n, reps):
    "the scoring kernel and the baseline on the same CSR and histories, alternately"
    import torch

    from lkpy_amd import _device as D

    s = scorer._device_scores()
    B = hist.shape[0]
    step = scorer._panel_rows()
    spans = [(lo, min(B, lo + step)) for lo in range(0, B, step)]

    def run(score, top):
        def go():
            for lo, hi in spans:
                panel = score(lo, hi)
                if top:
                    D.take_scores(panel, D.argtopn(panel, n))
        return go

    kinds = {
        "assoc_mean": lambda lo, hi: D.assoc_score_batch(
            hist.indptr, hist.indices, s, "mean", rows=(lo, hi), strike_history=True),
        "assoc_max": lambda lo, hi: D.assoc_score_batch(
            hist.indptr, hist.indices, s, "max", rows=(lo, hi), strike_history=True),
        "slim_baseline": lambda lo, hi: D.slim_score_batch(
            hist.indptr, hist.indices, s, rows=(lo, hi), strike_history=True, nan_empty=True),
    }
    # the same sums: baseline row / m in float64 == the mean panel, bit for bit
    lo, hi = spans[0][0], min(spans[0][1], 64)
    mean = D.assoc_score_batch(hist.indptr, hist.indices, s, "mean", rows=(lo, hi))
    sums = D.slim_score_batch(hist.indptr, hist.indices, s, rows=(lo, hi))
    m = (hist.indptr[lo + 1:hi + 1] - hist.indptr[lo:hi]).double().clamp(min=1).unsqueeze(1)
    same = bool(torch.equal((sums.double() / m).float(), mean))
    times = {f"{k}{suffix}": [] for k in kinds for suffix in ("", "+argtopn")}
    for rep in range(reps + 1):
        for top in (False, True):
            for k, score in kinds.items():
                t = _events(run(score, top))
                if rep:
                    times[k + ("+argtopn" if top else "")].append(t)
    lens = (s.indptr[1:] - s.indptr[:-1])
    entries = int(lens[hist.indices.long().clamp(min=0)].sum())
    n_bytes = 8 * entries + 4 * B * int(s.shape[1])
    out = {"queries": int(B), "panels": len(spans), "reference_items": int(hist.nnz),
           "row_entries_read": entries, "kernel_bytes": n_bytes,
           "mean_equals_baseline_sums_over_m": same}
    for k, ts in times.items():
        out[k] = _summary(ts)
        if "+" not in k:
            out[k]["bytes_per_s"] = round(n_bytes / out[k]["median_s"], 1)
    base = out["slim_baseline"]
    out["baseline_spread_s"] = round(base["max_s"] - base["min_s"], 6)
    out["mean_minus_baseline_s"] = round(out["assoc_mean"]["median_s"] - base["median_s"], 6)
    return out


def host_loop(scores, histories, n, max_lists, limit):
    "the per-query loop of the reference on this host: densify, mean, strike, top-n"
    t0 = time.perf_counter()
    done = 0
    for refs in histories[:max_lists]:
        dense = scores[refs, :].todense()
        row = np.mean(dense, axis=0)
        row[refs] = -np.inf
        top = np.argpartition(-row, n)[:n]
        top[np.argsort(-row[top], kind="stable")]
        done += 1
        if time.perf_counter() - t0 > limit:
            break
    return done, time.perf_counter() - t0


def recommend_legs(ds, users, n, reps, host_lists, host_limit):
    import torch

    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(ROOT / "tests" / "golden" / "pipelines" / "biased-lift.toml")
    t_train = _wall(lambda: pipe.train(ds), 1)[0]
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    batch = lookup.batch(users)
    out = {"pipeline_train_seconds": round(t_train, 4),
           "stored_pairs": int(scorer.assoc_scores.nnz), "users": int(len(users)), "n": n}
    mean_cfg = scorer.config
    for name, cfg in (("mean", mean_cfg), ("max", mean_cfg.model_copy(update={"max_nbrs": 1}))):
        scorer.config = cfg
        scorer.recommend_batch(lookup.batch(users[:64]), n)  # warm-up
        out[f"recommend_batch_{name}"] = r = _summary(
            _wall(lambda: scorer.recommend_batch(batch, n), reps))
        r["users_per_s"] = round(len(users) / r["median_s"], 1)
    scorer.config = mean_cfg
    out["kernels"] = score_legs(scorer, batch.csr(with_values=False), n, reps)
    torch.cuda.synchronize()
    hp = ds._indptr
    nums = batch.user_nums
    hists = [ds._cols[hp[u]:hp[u + 1]] for u in nums if u >= 0]
    done, secs = host_loop(scorer.assoc_scores, hists, n, host_lists, host_limit)
    out["host_loop"] = {
        "what": "per-query densify + np.mean + strike + top-n on this host; the batch figure is "
                "EXTRAPOLATED from the lists done, not measured",
        "lists_done": done, "seconds": round(secs, 3),
        "extrapolated_batch_seconds": round(secs / max(done, 1) * len(users), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--host-lists", type=int, default=2000)
    ap.add_argument("--host-limit", type=float, default=60.0)
    ap.add_argument("--commit", default=None, help="what the capture was taken from")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "capture_commit": args.commit,
           "window_columns": D.assoc_window()}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    rate, spread = copy_rate(dev)
    res["device_copy"] = {"bytes_per_s": rate, **spread}
    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    small = {"train": train_split(ds.interaction_matrix(), dev, 5)}
    users = ds.users.ids()
    small["recommend"] = recommend_legs(ds, users, 100, 5, args.host_lists, args.host_limit)
    res["ml_latest_small"] = small
    emit()

    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        big = {"train": train_split(ratings, dev, 3)}
        res["ml25m_like"] = big
        emit()
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        dset = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                       Vocabulary(np.arange(n_i), "item", reorder=False),
                       rows, ratings.indices, {"rating": ratings.data})
        users = np.random.default_rng(43).choice(n_u, min(args.users, n_u), replace=False)
        big["recommend"] = recommend_legs(dset, users, 100, 3, args.host_lists, args.host_limit)
    print(emit())


if __name__ == "__main__":
    main()
