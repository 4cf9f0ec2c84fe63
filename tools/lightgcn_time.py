#!/usr/bin/env python3
"""
Timing driver of the LightGCN trainer (csrc/lightgcn.hip, ``lkpy_amd.graphs.lightgcn``).

    python tools/lightgcn_time.py [--out FILE] [--no-ml25m] [--no-torch]

On ml-latest-small and on the ML-25M-shaped synthetic of ``bench.py``
(``lkpy_amd.synth.ml25m_like``), at k = 64 and L = 3 layers, pairwise loss, batches of 4 096:

* the training step (``LightGCNTrainer.train_batch``: gather, negatives, 2 L propagate launches,
  pair gradient, dense AdamW): the best of three timed runs of ``--steps`` steps after a warm-up.
  An epoch of ml-latest-small is timed whole (``train_epoch``, best of three); an epoch of the
  large shape is 6 104 steps, so it is reported as steps x the measured step time and marked as
  extrapolated.
* ``lk_lgcn_propagate`` alone (the fused ``a x + b M^ t`` pass): seconds per launch, the gathered
  bytes ``2 nnz (4 ld + 8)`` per second and the same with the streamed ``8 N ld`` bytes added.
  This is a host clock around 50 back-to-back launches through the Python wrapper, not a kernel
  trace: where a launch is shorter than the wrapper's own cost per call (ml-latest-small) the
  figure is an upper bound on the kernel time set by that overhead, and is marked so.
* the same step in Torch on the same GPU -- a sparse COO ``M^``, autograd through
  ``torch.sparse.mm``, ``torch.optim.AdamW`` -- if Torch's sparse product runs there; otherwise
  the exception it raised.
Times are host clocks around calls that end in a device synchronise.  One JSON document.
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

K, LAYERS, BATCH = 64, 3, 4096


def _best(fn, reps=3):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def _device_leg(ds, steps, whole_epoch):
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.training import TrainingOptions

    sc = LightGCNScorer(embedding_size=K, layer_count=LAYERS, batch_size=BATCH, epochs=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = sc.create_trainer(ds, TrainingOptions(rng=1))
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    st = tr.state
    n, ld, nnz = st.n, st.X.shape[1], st.indices.numel()
    perm = torch.from_numpy(np.random.default_rng(2).permutation(tr.n_samples).astype(np.int32))
    d_perm = perm.to(tr.dev)
    loss_sum = torch.zeros(1, dtype=torch.float32, device=tr.dev)
    steps = min(steps, (tr.n_samples + BATCH - 1) // BATCH)

    def run_steps():
        for b in range(steps):
            tr.train_batch(d_perm[b * BATCH:(b + 1) * BATCH], b, loss_sum)

    run_steps()  # warm-up: the workspace, the kernels' first launches
    step_best, step_all = _best(run_steps)
    out = {"k": K, "layers": LAYERS, "batch_size": BATCH, "nodes": int(n), "ld": int(ld),
           "adjacency_entries": int(nnz), "samples": int(tr.n_samples),
           "setup_seconds": round(setup, 4),
           "setup_what": "create_trainer: upload, transpose, adjacency, initial table",
           "steps_timed": steps, "step_seconds": round(step_best / steps, 7),
           "steps_seconds_all": [round(t, 6) for t in step_all]}
    epoch_steps = (tr.n_samples + BATCH - 1) // BATCH
    if whole_epoch:
        tr.train_epoch()
        best, every = _best(tr.train_epoch)
        out["epoch"] = {"steps": epoch_steps, "seconds": round(best, 5),
                        "seconds_all": [round(t, 5) for t in every], "extrapolated": False}
    else:
        out["epoch"] = {"steps": epoch_steps, "seconds": round(epoch_steps * step_best / steps, 3),
                        "extrapolated": True,
                        "what": "steps x the measured step time; not run as a whole"}
    # the propagate kernel alone
    t = st._work[2]
    t.copy_(st.X)
    reps = 50
    D.lgcn_propagate(st.indptr, st.indices, st.scale, 0.25, st.X, 1.0, t, K, st._work[0])

    def run_prop():
        for _ in range(reps):
            D.lgcn_propagate(st.indptr, st.indices, st.scale, 0.25, st.X, 1.0, t, K, st._work[0])

    best, _ = _best(run_prop)
    gathered = nnz * (4 * ld + 8)
    streamed = 8 * n * ld
    # the wrapper alone: the same call rejected before the launch (k = 0), so only host cost
    def run_wrapper():
        for _ in range(reps):
            try:
                D.lgcn_propagate(st.indptr, st.indices, st.scale, 0.25, st.X, 1.0, t, 0,
                                 st._work[0])
            except ValueError:
                pass

    wrapper, _ = _best(run_wrapper)
    out["propagate"] = {"seconds": round(best / reps, 7),
                        "what": f"host clock around {reps} back-to-back launches / {reps}",
                        "host_wrapper_seconds_per_call": round(wrapper / reps, 7),
                        "overhead_bound": bool(best < 4 * wrapper),
                        "gathered_bytes": int(gathered),
                        "streamed_bytes": int(streamed),
                        "gathered_gb_per_s": round(gathered / (best / reps) / 1e9, 1),
                        "all_bytes_gb_per_s": round((gathered + streamed) / (best / reps) / 1e9, 1),
                        "share_of_step": round(2 * LAYERS * best / reps / (step_best / steps), 3)}
    return out, tr


def _torch_leg(tr, steps):
    "the same step with Torch's own sparse product, autograd and AdamW on the same device"
    import torch

    try:
        st = tr.state
        dev = tr.dev
        rows = torch.repeat_interleave(torch.arange(st.n, device=dev),
                                       st.indptr[1:] - st.indptr[:-1])
        cols = st.indices.long()
        mhat = torch.sparse_coo_tensor(torch.stack([rows, cols]), st.scale[rows] * st.scale[cols],
                                       (st.n, st.n)).coalesce()
        X = torch.nn.Parameter(st.X[:, :K].clone())
        opt = torch.optim.AdamW([X], lr=0.01, weight_decay=0.01)
        alpha = 1.0 / (LAYERS + 1)
        rng = np.random.default_rng(3)
        sel = torch.from_numpy(rng.integers(0, tr.n_samples, (steps, BATCH))).to(dev)
        negs = torch.from_numpy(rng.integers(0, tr.n_items, (steps, BATCH))).to(dev)
        users, items = tr.d_users.long(), tr.d_items.long()

        def run():
            for b in range(steps):
                layer = X
                xbar = alpha * layer
                for _ in range(LAYERS):
                    layer = torch.sparse.mm(mhat, layer)
                    xbar = xbar + alpha * layer
                u = xbar[users[sel[b]]]
                sp = (u * xbar[items[sel[b]]]).sum(-1)
                sn = (u * xbar[negs[b]]).sum(-1)
                torch.nn.functional.softplus(sn - sp).mean().backward()
                opt.step()
                opt.zero_grad()

        run()
        best, every = _best(run)
        return {"ran": True, "what": "sparse COO M^, torch.sparse.mm with autograd, "
                "torch.optim.AdamW; given indices, no sampler", "steps_timed": steps,
                "step_seconds": round(best / steps, 7),
                "steps_seconds_all": [round(t, 6) for t in every]}
    except (RuntimeError, NotImplementedError, TypeError) as e:  # Torch's own refusals
        return {"ran": False, "error": f"{type(e).__name__}: {e}"[:500]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "spmm_split": D.spmm_split()}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    res["ml_latest_small"], tr_small = _device_leg(ds, args.steps, whole_epoch=True)
    emit()
    tr_big = None
    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        dset = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                       Vocabulary(np.arange(n_i), "item", reorder=False),
                       rows, ratings.indices, {"rating": ratings.data})
        res["ml25m_like"], tr_big = _device_leg(dset, args.steps, whole_epoch=False)
        emit()
    legs = [("ml_latest_small", tr_small)] + ([("ml25m_like", tr_big)] if tr_big else [])
    failed = None
    for name, tr in legs:
        if args.no_torch:
            res[name]["torch_same_gpu"] = {"ran": False, "error": "not asked for (--no-torch)"}
        elif failed is not None:  # nothing more is started on a device after a failed leg
            res[name]["torch_same_gpu"] = {"ran": False,
                                           "error": f"not started: the {failed} leg failed"}
        else:
            res[name]["torch_same_gpu"] = _torch_leg(tr, args.steps)
            if not res[name]["torch_same_gpu"]["ran"]:
                failed = name
        emit()
    print(emit())


if __name__ == "__main__":
    main()
