#!/usr/bin/env python3
"""
Timing driver of FlexMF explicit (``lkpy_amd.flexmf.FlexMFExplicitScorer``; csrc/flexmf.hip,
csrc/mf_pairs.hip) on the device.

    python tools/flexmf_explicit_time.py [--out profiles/flexmf_explicit_mi355x.json] [--no-ml25m]

* a training epoch at the default configuration (k 64, batch 8192, L2 0.1, SparseAdam) on
  ml-latest-small (tests/golden/ml_small.npz) and on the ML-25M-shaped synthetic of ``bench.py``
  (``lkpy_amd.synth.ml25m_like``): ``FlexMFExplicitTrainer.train_epoch``, which ends in the
  epoch's one synchronisation;
* the same epochs by Torch on the same GPU: ``nn.Embedding(sparse=True)`` tables, the loss
  ``mse + reg * mean(b_u^2 + b_i^2 + |p_u| + |q_i|)``, autograd and ``torch.optim.SparseAdam``,
  batches indexed out of a device-resident permutation (the formulas of
  tests/flexmf_explicit_restatement.py, kept on the device; not the reference's own code);
* ``lk_mf_score_pairs`` from device-resident inputs on 10 000 queries x 100 targets and
  1 000 000 queries x 5 targets (62 423 items, k 64 + 3 bias columns; 162 541 users for the
  first, a million users each asked once for the second), with the bytes the algorithm needs
  (per score the item's 67 floats, its number and the output; per query the user's 67 floats,
  its row number and one offset) over the time.

Times are host clocks around work that ends in a device synchronise; one warm-up, then
``--reps`` repeats: the median, the minimum, the maximum and every value.  One JSON document.
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


def _stats(walls):
    return {"median_s": round(float(np.median(walls)), 6), "min_s": round(min(walls), 6),
            "max_s": round(max(walls), 6), "all_s": [round(w, 6) for w in walls]}


def _timed(fn, reps):
    import torch

    fn()  # warm-up
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return _stats(walls)


def device_epochs(ds, reps):
    from lkpy_amd.flexmf import FlexMFExplicitScorer
    from lkpy_amd.training import TrainingOptions

    tr = FlexMFExplicitScorer().create_trainer(ds, TrainingOptions(rng=1))
    losses = []
    out = _timed(lambda: losses.append(tr.train_epoch()["loss"]), reps)
    out["epoch_losses"] = [round(v, 6) for v in losses]
    return out


def torch_epochs(ds, dev, reps, cfg):
    "the restatement's epoch with everything on the device"
    import torch
    from torch import nn
    from torch.nn import functional as F

    from lkpy_amd.flexmf import centred_ratings, initial_tables

    gen = torch.Generator().manual_seed(1)
    tabs = initial_tables(ds.user_count, ds.item_count, cfg.embedding_size, gen, user_bias=True,
                          item_bias=True)
    emb = {}
    for name, w in tabs.items():
        e = nn.Embedding(w.shape[0], w.shape[1], sparse=True, device=dev)
        with torch.no_grad():
            e.weight.copy_(torch.from_numpy(w))
        emb[name.split(".")[0]] = e
    opt = torch.optim.SparseAdam([e.weight for e in emb.values()], lr=cfg.learning_rate)
    users = torch.from_numpy(ds._rows.astype(np.int64)).to(dev)
    items = torch.from_numpy(ds._cols.astype(np.int64)).to(dev)
    ratings = torch.from_numpy(centred_ratings(ds)[1]).to(dev)
    rng = np.random.default_rng(1)
    losses = []

    def epoch():
        perm = torch.from_numpy(rng.permutation(len(ds._rows))).to(dev)
        total = torch.zeros((), device=dev)
        n = 0
        for s in range(0, len(perm), cfg.batch_size):
            sel = perm[s:s + cfg.batch_size]
            u, i = users[sel], items[sel]
            p, q = emb["u_embed"](u), emb["i_embed"](i)
            bu, bi = emb["u_bias"](u).squeeze(-1), emb["i_bias"](i).squeeze(-1)
            mse = F.mse_loss(bu + bi + (p * q).sum(-1), ratings[sel])
            norm = (bu * bu + bi * bi + p.norm(dim=-1) + q.norm(dim=-1)).mean()
            (mse + cfg.regularization * norm).backward()
            opt.step()
            opt.zero_grad()
            total += mse.detach()
            n += 1
        losses.append(float(total.item()) / n)

    out = _timed(epoch, reps)
    out["epoch_losses"] = [round(v, 6) for v in losses]
    return out


def pair_scoring(dev, n_queries, per_query, reps, n_users=162541, n_items=62423, k=64):
    import torch

    from lkpy_amd import _device as D

    ks = k + 3
    kp = D.padded_dim(ks)
    g = torch.Generator(device=dev).manual_seed(7)
    U = torch.zeros((n_users, kp), device=dev)
    Q = torch.zeros((n_items, kp), device=dev)
    U[:, :ks] = torch.randn((n_users, ks), device=dev, generator=g)
    Q[:, :ks] = torch.randn((n_items, ks), device=dev, generator=g)
    if n_queries == n_users:  # every user once
        rows = torch.randperm(n_users, device=dev, generator=g).to(torch.int32)
    else:
        rows = torch.randint(0, n_users, (n_queries,), device=dev, generator=g, dtype=torch.int32)
    tgts = torch.randint(0, n_items, (n_queries * per_query,), device=dev, generator=g,
                         dtype=torch.int32)
    ptr = torch.arange(n_queries + 1, device=dev, dtype=torch.int64) * per_query
    out = _timed(lambda: D.mf_score_pairs(U, Q, ks, rows, ptr, tgts), reps)
    scores = n_queries * per_query
    nbytes = scores * (4 * ks + 8) + n_queries * (4 * ks + 12)
    out.update(queries=n_queries, targets_per_query=per_query, inner_width=ks,
               row_stride_bytes=4 * kp, bytes_needed=nbytes, bytes_per_score=round(nbytes / scores, 1),
               achieved_GBps=round(nbytes / out["median_s"] / 1e9, 1),
               item_table_MB=round(n_items * kp * 4 / 1e6, 1),
               user_table_MB=round(n_users * kp * 4 / 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz
    from lkpy_amd.flexmf import FlexMFExplicitConfig

    dev = D.device()
    cfg = FlexMFExplicitConfig()
    res = {"device": torch.cuda.get_device_name(dev), "repeats": args.reps,
           "config": cfg.model_dump()}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    res["score_pairs_10000x100"] = pair_scoring(dev, 10_000, 100, args.reps)
    res["score_pairs_1000000x5"] = pair_scoring(dev, 1_000_000, 5, args.reps, n_users=1_000_000)
    emit()

    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    res["ml_latest_small"] = {
        "shape": [ds.user_count, ds.item_count], "ratings": int(ds.interaction_count),
        "batches_per_epoch": -(-ds.interaction_count // cfg.batch_size),
        "device_epoch": device_epochs(ds, args.reps),
        "torch_epoch_same_gpu": torch_epochs(ds, dev, args.reps, cfg)}
    emit()

    if not args.no_ml25m:
        from lkpy_amd import synth

        mat = synth.ml25m_like()
        n_u, n_i = mat.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(mat.indptr))
        big = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                      Vocabulary(np.arange(n_i), "item", reorder=False), rows,
                      mat.indices.astype(np.int32), {"rating": mat.data.astype(np.float32)})
        res["ml25m_like"] = {
            "shape": [n_u, n_i], "ratings": int(mat.nnz),
            "batches_per_epoch": -(-int(mat.nnz) // cfg.batch_size)}
        res["ml25m_like"]["device_epoch"] = device_epochs(big, args.reps)
        emit()
        res["ml25m_like"]["torch_epoch_same_gpu"] = torch_epochs(big, dev, args.reps, cfg)
    print(emit())


if __name__ == "__main__":
    main()
