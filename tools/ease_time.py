#!/usr/bin/env python3
"""
Timing driver of EASE's training and batch recommendation on the device
(csrc/spd_blocked.hip, ``lk_ease_score_panel``).

    python tools/ease_time.py [--out FILE] [--ml25m | --only-ml25m] [--no-library-ml25m]
                              [--users N] [--loop-users N] [--commit TEXT]

* ``lk_gemm_f32`` alone: an 8192^3 product per op form the inverse uses (NT, NN, TN), 2 m n k
  flops over the device-event time;
* the SPD inverse of the EASE Gramian, ``native`` (``lk_spd_inverse_blocked``) and ``torch``
  (``cholesky_ex`` + ``cholesky_inverse``), alternately on copies of the same matrix, each repeat
  listed; the ``native`` run again as its three phases (``lk_spd_inverse_blocked_phases``) with a
  device event between them, and each phase's n^3 / 3 flops over its time; the distance between
  the two inverses;
* ``EASEScorer.train`` end to end (co-occurrences, Gramian, inverse, scaling, download) for both
  solvers -- on ml-latest-small (tests/golden/ml_small.npz), and with ``--ml25m`` the
  inverse legs on the Gramian of the ML-25M-shaped synthetic of ``lkpy_amd.synth.ml25m_like``
  (62 423 items: two 15.6 GB matrices per solver; the end-to-end training is not repeated there);
* ``recommend_batch`` top-100 for ``--users`` users against ``batch._recommend_loop`` (one
  pipeline run per user) over ``--loop-users`` users, EXTRAPOLATED to the batch and named so.
Times are device events around queued work, host clocks around calls that end in a device
synchronise; every timed shape is run once before it is timed.  One JSON document, rewritten
after every stage.
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


def gemm_rates(dev, size, reps):
    "TF/s of lk_gemm_f32 alone, per op form of the inverse"
    import torch

    from lkpy_amd import _device as D

    a = torch.randn((size, size), dtype=torch.float32, device=dev)
    b = torch.randn((size, size), dtype=torch.float32, device=dev)
    c = torch.empty((size, size), dtype=torch.float32, device=dev)
    out = {"m_n_k": size, "flops": 2 * size ** 3}
    for name, ta, tb in (("NT", False, True), ("NN", False, False), ("TN", True, False)):
        run = lambda: D.gemm_f32(a, b, c, trans_a=ta, trans_b=tb)  # noqa: E731
        run()
        ts = [_events(run) for _ in range(reps)]
        out[name] = {**_summary(ts),
                     "tflops": round(2 * size ** 3 / statistics.median(ts) / 1e12, 2)}
    return out


def _torch_inverse(g):
    import torch

    decomp, info = torch.linalg.cholesky_ex(g)
    inv = torch.cholesky_inverse(decomp, out=g)
    return inv, info


def _native_phases(a):
    "one inversion as three calls, an event after each: seconds of (a), (b), (c)"
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    lib = _native.require_gpu()
    n = int(a.shape[0])
    nbytes = int(lib.lk_spd_inverse_blocked_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    flag = torch.zeros(1, dtype=torch.int32, device=a.device)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    marks[0].record()
    for i, phase in enumerate((1, 2, 4)):
        _native.check(lib.lk_spd_inverse_blocked_phases(D._ptr(a), n, n, D._ptr(ws), nbytes,
                                                        D._ptr(flag), phase, D._stream()),
                      "lk_spd_inverse_blocked_phases")
        marks[i + 1].record()
    marks[3].synchronize()
    assert int(flag.item()) == 0
    return [marks[i].elapsed_time(marks[i + 1]) * 1e-3 for i in range(3)]


def inverse_legs(gram, reps, out, emit=lambda: None, library=True):
    """native and torch on copies of ``gram``, alternately; then the native phases.  Fills ``out``
    as it goes and calls ``emit`` after every timed call (a large matrix takes a while).  A library
    call that raises is recorded with its message and not repeated; ``library=False`` leaves the
    library legs out."""
    import torch

    from lkpy_amd import _device as D

    n = int(gram.shape[0])
    work = torch.empty_like(gram)
    times = {"native": [], "torch": []}
    keep = {}
    out.update({"n": n, "flops_n3": n ** 3})
    if not library:
        out["torch"] = {"skipped": "--no-library-ml25m"}
    for rep in range(reps + 1):  # (the first pass is the warm-up, listed apart)
        for name in ("native", "torch"):
            if name == "torch" and "torch" in out and "median_s" not in out["torch"]:
                continue
            work.copy_(gram)
            if name == "native":
                t = _events(lambda: D.spd_inverse_blocked(work))
            else:
                try:
                    t = _events(lambda: _torch_inverse(work))
                except RuntimeError as e:
                    out["torch"] = {"error": str(e).splitlines()[0]}
                    emit()
                    continue
            if rep:
                times[name].append(t)
                out[name] = _summary(times[name])
            else:
                out[f"{name}_first_call_s"] = round(t, 6)
                if name == "native":  # the last 128 rows of G G^-1 - I (plumbing: a Torch product)
                    r = gram[-128:] @ work
                    r[:, -r.shape[0]:] -= torch.eye(r.shape[0], device=r.device)
                    out["native_max_abs_residual_last_rows"] = float(r.abs().max())
                if n <= 16384:
                    keep[name] = work.clone()
            emit()
    if len(keep) == 2:
        out["rel_frobenius_native_vs_torch"] = float(
            torch.linalg.norm(keep["native"].double() - keep["torch"].double()) /
            torch.linalg.norm(keep["torch"].double()))
    keep.clear()
    phases = []
    for _ in range(max(1, reps)):
        work.copy_(gram)
        phases.append(_native_phases(work))
    third = n ** 3 / 3
    for i, name in enumerate(("a_factorise", "b_invert_factor", "c_product")):
        ts = [p[i] for p in phases]
        out[f"phase_{name}"] = {**_summary(ts), "flops": round(third),
                                "tflops": round(third / statistics.median(ts) / 1e12, 2)}
    emit()
    return out


def gramian(ratings, dev, reg=1.0):
    import scipy.sparse as sps
    import torch

    from lkpy_amd import _device as D

    ui = sps.csr_array(ratings).astype(np.float32)
    ui.sum_duplicates()
    ui.data[:] = 1.0
    ui.sort_indices()
    iu = sps.csr_array(ui.T)
    iu.sort_indices()
    cooc = D.iknn_build(D.DeviceCSR.from_scipy(ui, dev), D.DeviceCSR.from_scipy(iu, dev), 0.5)
    counts = torch.from_numpy(np.diff(iu.indptr).astype(np.int32)).to(dev)
    return D.ease_gram(cooc, counts, reg)


def train_legs(ds, reps):
    "EASEScorer.train end to end, both solvers alternately"
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.training import TrainingOptions

    times = {"native": [], "torch": []}
    for rep in range(reps + 1):
        for name in times:
            opts = TrainingOptions(environment={"LK_EASE_SOLVER": name})
            t = _wall(lambda: EASEScorer().train(ds, opts), 1)[0]
            if rep:
                times[name].append(t)
    return {k: _summary(v) for k, v in times.items()}


def recommend_legs(ds, users, n, reps, loop_users):
    from lkpy_amd import batch
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.pipeline import topn_pipeline

    pipe = topn_pipeline(EASEScorer())
    pipe.train(ds)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    hb = lookup.batch(users)
    scorer.recommend_batch(lookup.batch(users[:64]), n)  # warm-up
    out = {"users": int(len(users)), "n": n, "items": int(len(scorer.items)),
           "panel_rows": int(scorer._panel_rows())}
    out["recommend_batch"] = r = _summary(_wall(lambda: scorer.recommend_batch(hb, n), reps))
    r["users_per_s"] = round(len(users) / r["median_s"], 1)
    some = [u.item() for u in users[:loop_users]]
    batch._recommend_loop(pipe, some[:8], n)  # warm-up
    secs = _wall(lambda: batch._recommend_loop(pipe, some, n), 1)[0]
    out["recommend_loop"] = {
        "what": "batch._recommend_loop, one pipeline run per user; the batch figure is "
                "EXTRAPOLATED from the users done, not measured",
        "users_done": len(some), "seconds": round(secs, 3),
        "extrapolated_batch_seconds": round(secs / max(len(some), 1) * len(users), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ml25m", action="store_true", help="also the ML-25M-shaped inverse (31 GB)")
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--loop-users", type=int, default=2000)
    ap.add_argument("--gemm-size", type=int, default=8192)
    ap.add_argument("--only-ml25m", action="store_true", help="skip the ml-latest-small legs")
    ap.add_argument("--no-library-ml25m", action="store_true",
                    help="at the ML-25M shape time the native inverse only")
    ap.add_argument("--commit", default=None, help="what the capture was taken from")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D

    dev = D.device()
    res = {"device": torch.cuda.get_device_name(dev), "capture_commit": args.commit,
           "block": D.gemm_tile()}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    if args.only_ml25m:
        args.ml25m = True
    else:
        small_legs(args, res, dev, emit)

    if args.ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        res["ml25m_like"] = {"shape": list(map(int, ratings.shape)),
                             "interactions": int(ratings.nnz)}
        emit()
        g = gramian(ratings, dev)
        torch.cuda.synchronize()
        res["ml25m_like"]["inverse"] = {}
        inverse_legs(g, 1, res["ml25m_like"]["inverse"], emit, library=not args.no_library_ml25m)
    print(emit())


def small_legs(args, res, dev, emit):
    from lkpy_amd.data import load_movielens_npz

    res["gemm_f32"] = gemm_rates(dev, args.gemm_size, 5)
    emit()
    ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    small = {"inverse": {}}
    res["ml_latest_small"] = small
    inverse_legs(gramian(ds.interaction_matrix(), dev), 5, small["inverse"], emit)
    small["train"] = train_legs(ds, 3)
    emit()
    ids = ds.users.ids()
    users = ids[np.arange(args.users) % len(ids)]  # (610 users: repeated up to the batch size)
    small["recommend"] = recommend_legs(ds, users, 100, 5, args.loop_users)
    emit()


if __name__ == "__main__":
    main()
