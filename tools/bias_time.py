#!/usr/bin/env python3
"""
Timing driver of the bias model on the device (csrc/bias.hip).

    python tools/bias_time.py [--out profiles/bias_mi355x.json] [--no-ml25m] [--no-trainers]

On ml-latest-small and on the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``):

* the fit: ``BiasModel.learn`` on the host (the ``np.add.at`` arithmetic, on THIS host's CPU) beside
  ``learn(device=...)`` end to end (upload, transpose, both passes, download) and its parts -- the
  upload, ``csr_transpose``, the two ``lk_bias_fit_pass`` calls alone (best of five, matrices
  already in HBM) --, a device copy of the ratings as the bandwidth yardstick, and the longest
  item's bin fitted alone (a one-bin CSR): the latency of one chain, which is what bounds the pass;
  that the two models have the same bits is checked on the way;
* ``BiasedSVDScorer.train`` and a one-epoch ``BiasedMFScorer`` training with the fit on the device,
  and the same training with the host fit in its place (``BiasModel.learn`` made to ignore
  ``device``: the trainers as they ran before), each the best of two after a warm-up run;
* ``batch.predict`` (20 targets a user), ``batch.score`` (100 candidates a user) and
  ``batch.recommend`` (n = 100) over a trained Bias pipeline for 10 000 users, each beside the
  ``pipe.run`` loop timed on 500 users and scaled.
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

DAMPING = 100 / 3


def _best(fn, reps=5):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(min(ts), 6), [round(t, 6) for t in ts]


def _fit(ds, dev):
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.basic import BiasModel

    ratings = ds._attrs["rating"]
    n_u, n_i, nnz = ds.user_count, ds.item_count, len(ratings)
    t0 = time.perf_counter()
    host = BiasModel.learn(ds, DAMPING)
    t_host = time.perf_counter() - t0
    BiasModel.learn(ds, DAMPING, device=dev)  # warm-up: module load, allocator
    e2e, e2e_all = _best(lambda: BiasModel.learn(ds, DAMPING, device=dev), 3)
    got = BiasModel.learn(ds, DAMPING, device=dev)
    same = bool(np.array_equal(got.item_biases.view(np.uint32), host.item_biases.view(np.uint32))
                and np.array_equal(got.user_biases.view(np.uint32),
                                   host.user_biases.view(np.uint32)))
    up, _ = _best(lambda: D.DeviceCSR.from_arrays(ds._indptr, ds._cols, ratings, (n_u, n_i), dev), 3)
    csr = D.DeviceCSR.from_arrays(ds._indptr, ds._cols, ratings, (n_u, n_i), dev)
    tr, _ = _best(lambda: D.csr_transpose(csr, with_values=True), 3)
    csr_t = D.csr_transpose(csr, with_values=True)
    g = host.global_bias
    both, both_all = _best(lambda: D.bias_fit(csr, csr_t, g, DAMPING, DAMPING))
    items_only, _ = _best(lambda: D.bias_fit(csr, csr_t, g, DAMPING, DAMPING, users=False))
    ib = D.bias_fit(csr, csr_t, g, DAMPING, DAMPING, users=False)[0]
    users_only, _ = _best(lambda: _user_pass(D, csr, g, ib))
    copy, _ = _best(lambda: csr.values.clone())
    # the longest item's bin alone
    lens = np.bincount(ds._cols, minlength=n_i)
    top = int(lens.argmax())
    t_ptr = csr_t.indptr.cpu().numpy()
    s, e = int(t_ptr[top]), int(t_ptr[top + 1])
    one = D.DeviceCSR(torch.tensor([0, e - s], dtype=torch.int64, device=dev),
                      csr_t.indices[s:e].contiguous(), csr_t.values[s:e].contiguous(),
                      (1, n_u), None)
    lone, _ = _best(lambda: _one_bin(D, one, g))
    return {
        "shape": [n_u, n_i], "nnz": int(nnz), "damping": DAMPING,
        "longest_item": int(lens.max()), "longest_user": int(np.diff(ds._indptr).max()),
        "host_learn_seconds": round(t_host, 4),
        "device_learn_seconds": e2e, "device_learn_seconds_all": e2e_all,
        "device_learn_what": "learn(device=...): upload, transpose, both passes, download",
        "same_bits_as_host": same,
        "upload_seconds": up, "transpose_seconds": tr,
        "both_passes_seconds": both, "both_passes_seconds_all": both_all,
        "item_pass_seconds": items_only, "user_pass_seconds": users_only,
        "ratings_copy_seconds": copy,
        "ratings_copy_gb_per_s": round(8 * nnz / copy / 1e9, 1),
        "pass_bytes": {"item": int(4 * nnz + 8 * n_i), "user": int(8 * nnz + 8 * n_u)},
        "longest_item_chain_alone_seconds": lone,
    }


def _user_pass(D, csr, g, ib):
    from lkpy_amd._device import _ptr, _stream
    from lkpy_amd import _native
    import torch

    lib = _native.load()
    out = torch.empty(csr.shape[0], dtype=torch.float32, device=ib.device)
    D.check(lib.lk_bias_fit_pass(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                                 _ptr(csr.values), csr.shape[0], float(g), _ptr(ib),
                                 csr.shape[1], DAMPING, _ptr(out), _stream()),
            "lk_bias_fit_pass")
    return out


def _one_bin(D, one, g):
    from lkpy_amd._device import _ptr, _stream
    from lkpy_amd import _native
    import torch

    lib = _native.load()
    out = torch.empty(1, dtype=torch.float32, device=one.values.device)
    D.check(lib.lk_bias_fit_pass(_ptr(one.indptr), 1, _ptr(None), _ptr(one.values), 1, float(g),
                                 _ptr(None), 0, DAMPING, _ptr(out), _stream()),
            "lk_bias_fit_pass")
    return out


def _host_fit():
    "a context in which ``BiasModel.learn`` ignores ``device``: the trainers as they ran before"
    from contextlib import contextmanager

    from lkpy_amd.basic import BiasModel

    @contextmanager
    def ctx():
        orig = BiasModel.learn.__func__

        def learn(cls, data, damping=0.0, *, entities=("user", "item"), device=None, csr=None,
                  csr_t=None):
            return orig(cls, data, damping, entities=entities)

        BiasModel.learn = classmethod(learn)
        try:
            yield
        finally:
            BiasModel.learn = classmethod(orig)

    return ctx()


def _trainers(ds):
    import torch

    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.sklearn.svd import BiasedSVDScorer
    from lkpy_amd.training import TrainingOptions

    def once(make):
        sc = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.train(ds, TrainingOptions(rng=1))
        torch.cuda.synchronize()
        return round(time.perf_counter() - t0, 4)

    out = {}
    for name, make in (("BiasedSVDScorer", lambda: BiasedSVDScorer(features=64, damping=DAMPING)),
                       ("BiasedMFScorer_1_epoch",
                        lambda: BiasedMFScorer(embedding_size=64, epochs=1, damping=DAMPING))):
        once(make)  # warm-up: modules, allocator, plans
        after = [once(make) for _ in range(2)]
        with _host_fit():
            before = [once(make) for _ in range(2)]
        out[name] = {"train_seconds": min(after), "train_seconds_all": after,
                     "with_the_host_fit_seconds": min(before),
                     "with_the_host_fit_seconds_all": before}
    return out


def _batch_calls(ds):
    import torch

    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(ROOT / "tests" / "golden" / "pipelines" / "bias.toml")
    pipe.train(ds)
    rng = np.random.default_rng(43)
    n = min(10000, ds.user_count)
    uids = ds.users.ids()[rng.choice(ds.user_count, n, replace=False)]
    ids = ds.items.ids()
    loop_users = [u.item() for u in uids[:500]]

    def lists(k):
        picks = rng.integers(0, len(ids), (n, k))
        return {u.item(): ItemList(item_ids=ids[picks[b]]) for b, u in enumerate(uids)}

    out = {"users": int(n), "loop_users": len(loop_users)}
    pairs, cands = lists(20), lists(100)
    calls = {
        "predict_20_targets": (lambda: batch.predict(pipe, pairs),
                               lambda: [pipe.run("rating-predictor", query=u, items=pairs[u])
                                        for u in loop_users]),
        "score_100_candidates": (lambda: batch.score(pipe, cands),
                                 lambda: [pipe.run("scorer", query=u, items=cands[u])
                                          for u in loop_users]),
        "recommend_n100": (lambda: batch.recommend(pipe, uids, 100).lists(),
                           lambda: [pipe.run("recommender", query=u, n=100) for u in loop_users]),
    }
    for name, (whole, loop) in calls.items():
        whole()  # uploads
        t, t_all = _best(whole, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        t_loop = (time.perf_counter() - t0) * n / len(loop_users)
        out[name] = {"seconds": t, "seconds_all": t_all, "users_per_s": round(n / t, 1),
                     "pipe_run_loop_seconds_scaled": round(t_loop, 3),
                     "speedup": round(t_loop / t, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--no-trainers", action="store_true")
    args = ap.parse_args()

    import platform

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz

    dev = D.device()
    lib = _native.load()
    res = {"device": torch.cuda.get_device_name(dev), "host_cpu": platform.processor() or
           platform.machine(), "numpy": np.__version__,
           "short_max": int(lib.lk_bias_fit_short_max()), "chunk": int(lib.lk_bias_fit_chunk())}

    def emit():
        text = json.dumps(res, indent=1)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return text

    def run(name, ds):
        part = res[name] = {"fit": _fit(ds, dev)}
        emit()
        part["batch"] = _batch_calls(ds)
        emit()
        if not args.no_trainers:
            part["trainers"] = _trainers(ds)
            emit()

    run("ml_latest_small", load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz"))
    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        run("ml25m_like", Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                                  Vocabulary(np.arange(n_i), "item", reorder=False),
                                  rows, ratings.indices, {"rating": ratings.data}))
    print(emit())


if __name__ == "__main__":
    main()
