#!/usr/bin/env python3
"""
Timing driver of the hierarchical Poisson factorization trainer (csrc/hpf.hip,
``lkpy_amd.hpf``).

    python tools/hpf_time.py [--out FILE] [--no-ml25m] [--no-torch] [--host-large]

On ml-latest-small (ratings + 0.5 as counts) and on the ML-25M-shaped synthetic of ``bench.py``
(``lkpy_amd.synth.ml25m_like``, its ratings as counts), at k = 64:

* one iteration (``HPFState.iterate``: two ``lk_hpf_expect_log``, two ``lk_hpf_shape_pass``, two
  ``lk_hpf_rates``): the best of three timed runs of ``--iters`` queued iterations after a
  warm-up, and a whole ``HPFScorer.train`` of 100 iterations with the default stopping options
  switched to ``stop_crit="maxiter"`` and with them as they are;
* each kernel alone, device events around ``--reps`` back-to-back launches: the two expect-log
  passes, the shape pass on Y and on Y^T, the two rate passes, the log-likelihood rows;
* beside each shape pass, ``lk_csr_spmm`` on the same matrix with l = 64, alternating with it in
  the same loop: the yardstick for the gather.  The ratio and the gathered bytes
  ``nnz (4 ld + 8)`` per second of both;
* the same iteration written with Torch (``index_select``, ``softmax``, ``index_add_``) on the
  same GPU, or the exception Torch raised;
* the float32 restatement (tests/hpf_restatement.py) on the host: one iteration.  On the large
  shape it needs tens of GB and about a minute, so it runs there only with ``--host-large``.

Where a launch is shorter than the wrapper's own cost per call (ml-latest-small) a per-kernel
figure is an upper bound set by that overhead.  One JSON document.
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

K = 64


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


def _events(fns, reps):
    "seconds per launch of each of ``fns``, launched alternately ``reps`` times; best of three"
    import torch

    best = [float("inf")] * len(fns)
    for fn in fns:
        fn()  # warm-up
    for _ in range(3):
        tot = [0.0] * len(fns)
        marks = []
        for _ in range(reps):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                marks.append((i, a, b))
        torch.cuda.synchronize()
        for i, a, b in marks:
            tot[i] += a.elapsed_time(b) * 1e-3
        best = [min(x, t / reps) for x, t in zip(best, tot)]
    return best


def _start(shape, seed=1):
    import hpf_restatement as R

    return R.start_panels(shape[0], shape[1], K, np.random.default_rng(seed))


def _device_leg(mat, iters, reps):
    import torch

    from lkpy_amd import _device as D

    dev = D.device()
    y = mat.data.astype(np.float32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    csr = D.DeviceCSR.from_arrays(mat.indptr, mat.indices, y, mat.shape, dev)
    st = D.HPFState(csr, _start(mat.shape))
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    n_u, n_i = mat.shape
    nnz, ld = csr.nnz, st.g_shp.shape[1]
    st.iterate(2)  # warm-up
    best, every = _best(lambda: st.iterate(iters))
    out = {"k": K, "ld": int(ld), "users": int(n_u), "items": int(n_i), "entries": int(nnz),
           "longest_user_row": int(np.diff(mat.indptr).max()),
           "setup_seconds": round(setup, 4),
           "setup_what": "upload, lk_csr_transpose, the start's means and sums on the host",
           "iterations_timed": iters, "iteration_seconds": round(best / iters, 7),
           "iterations_seconds_all": [round(t, 6) for t in every]}
    _, ll = _best(st.loglik, reps=3)
    out["loglik_check_seconds"] = round(min(ll), 6)

    k = st.k
    scratch_u, scratch_i = torch.empty_like(st.g_shp), torch.empty_like(st.l_shp)
    k_rte, t_rte = st.k_rte.clone(), st.t_rte.clone()
    col_a, col_b = torch.empty_like(st.T), torch.empty_like(st.S)
    rte_u, mean_u = torch.empty_like(st.g_shp), torch.empty_like(st.g_shp)
    rte_i, mean_i = torch.empty_like(st.l_shp), torch.empty_like(st.l_shp)
    D.hpf_expect_log(st.g_shp, st.g_rte, k, st.e_u)
    D.hpf_expect_log(st.l_shp, st.l_rte, k, st.e_i)
    fns = {
        "expect_log_users": lambda: D.hpf_expect_log(st.g_shp, st.g_rte, k, scratch_u),
        "expect_log_items": lambda: D.hpf_expect_log(st.l_shp, st.l_rte, k, scratch_i),
        "shape_pass_users": lambda: D.hpf_shape_pass(st.csr, st.e_u, st.e_i, k, st.a, scratch_u),
        "spmm_users": lambda: D.csr_spmm(st.csr, st.e_i, k),
        "shape_pass_items": lambda: D.hpf_shape_pass(st.csr_t, st.e_i, st.e_u, k, st.c, scratch_i),
        "spmm_items": lambda: D.csr_spmm(st.csr_t, st.e_u, k),
        "rates_users": lambda: D.hpf_rates(st.g_shp, k, st.k_shp, st.k_ratio, k_rte, st.S, rte_u,
                                           mean_u, col_a, st._ws),
        "rates_items": lambda: D.hpf_rates(st.l_shp, k, st.t_shp, st.t_ratio, t_rte, st.T, rte_i,
                                           mean_i, col_b, st._ws),
        "loglik_rows": lambda: D.hpf_loglik_rows(st.csr, st.theta, st.beta, k),
    }
    secs = dict(zip(fns, _events(list(fns.values()), reps)))
    gathered = nnz * (4 * ld + 8)
    out["kernels"] = {"what": f"device events around each of {reps} launches, the kernels "
                      "launched alternately; best mean of three rounds",
                      "seconds": {n: round(s, 7) for n, s in secs.items()},
                      "gathered_bytes_per_pass": int(gathered)}
    for side in ("users", "items"):
        sp, mm = secs[f"shape_pass_{side}"], secs[f"spmm_{side}"]
        out["kernels"][f"shape_pass_{side}"] = {
            "gathered_gb_per_s": round(gathered / sp / 1e9, 1),
            "spmm_gathered_gb_per_s": round(gathered / mm / 1e9, 1),
            "shape_pass_over_spmm": round(sp / mm, 2)}
    six = sum(secs[n] for n in ("expect_log_users", "expect_log_items", "shape_pass_users",
                                "shape_pass_items", "rates_users", "rates_items"))
    out["kernels"]["sum_of_the_six_of_an_iteration"] = round(six, 7)

    def wrapper():
        for _ in range(reps):
            try:
                D.hpf_expect_log(st.g_shp, st.g_rte, k, st.g_shp[:0])
            except (AssertionError, ValueError):
                pass

    w, _ = _best(wrapper)
    out["kernels"]["host_wrapper_seconds_per_call"] = round(w / reps, 7)
    return out, st


def _train_leg(ds, count_attribute):
    "a whole HPFScorer.train: 100 iterations without checks, and the default stopping rule"
    import torch

    from lkpy_amd.hpf import HPFScorer
    from lkpy_amd.training import TrainingOptions

    out = {}
    for name, cfg in (("maxiter_100", dict(stop_crit="maxiter")), ("default_stopping", {})):
        sc = HPFScorer(features=K, count_attribute=count_attribute, **cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.train(ds, TrainingOptions(rng=1))
        torch.cuda.synchronize()
        out[name] = {"seconds": round(time.perf_counter() - t0, 4), "iterations": sc.n_iter_,
                     "loglik": [round(v, 3) for v in sc.loglik_],
                     "what": "HPFScorer.train whole: host matrix preparation, upload, fit, download"}
    return out


def _torch_leg(st, iters):
    "the same iteration with Torch's own kernels on the same device"
    import torch

    try:
        k, dev = st.k, st.dev
        ptr = st.csr.indptr.long()
        rows = torch.repeat_interleave(torch.arange(st.csr.shape[0], device=dev),
                                       ptr[1:] - ptr[:-1])
        cols, y = st.csr.indices.long(), st.csr.values
        g_shp, g_rte = st.g_shp[:, :k].clone(), st.g_rte[:, :k].clone()
        l_shp, l_rte = st.l_shp[:, :k].clone(), st.l_rte[:, :k].clone()
        k_rte, t_rte, S = st.k_rte.clone(), st.t_rte.clone(), st.S.clone()
        a, c = st.a, st.c

        def run():
            nonlocal g_shp, g_rte, l_shp, l_rte, k_rte, t_rte, S
            for _ in range(iters):
                e_u = torch.digamma(g_shp) - torch.log(g_rte)
                e_i = torch.digamma(l_shp) - torch.log(l_rte)
                phi = torch.softmax(e_u.index_select(0, rows) + e_i.index_select(0, cols), dim=1)
                phi *= y[:, None]
                g_shp = torch.full_like(g_shp, a).index_add_(0, rows, phi)
                l_shp = torch.full_like(l_shp, c).index_add_(0, cols, phi)
                del phi
                g_rte = (st.k_shp / k_rte)[:, None] + S[None, :]
                theta = g_shp / g_rte
                k_rte = st.k_ratio + theta.sum(1)
                l_rte = (st.t_shp / t_rte)[:, None] + theta.sum(0)[None, :]
                beta = l_shp / l_rte
                t_rte = st.t_ratio + beta.sum(1)
                S = beta.sum(0)

        run()
        best, every = _best(run)
        return {"ran": True, "what": "float32 digamma / log, index_select, softmax, index_add_ "
                "(atomic adds: the sums' order is not fixed), one phi for both sides",
                "iterations_timed": iters, "iteration_seconds": round(best / iters, 7),
                "iterations_seconds_all": [round(t, 6) for t in every]}
    except (RuntimeError, NotImplementedError, TypeError) as e:  # Torch's own refusals
        return {"ran": False, "error": f"{type(e).__name__}: {e}"[:500]}


def _mem_available_gb() -> float:
    try:
        for line in Path("/proc/meminfo").read_text().splitlines():
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


def _host_leg(mat, reps):
    import hpf_restatement as R

    need = 6 * mat.nnz * K * 4 / 2 ** 30  # about six [entries x k] float32 arrays alive at once
    if _mem_available_gb() < 2 * need:
        return {"ran": False, "error": f"not started: about {need:.0f} GB of host memory needed, "
                f"{_mem_available_gb():.0f} GB available"}

    trip = R.coo_of(mat)
    st = R.init_state(_start(mat.shape), dtype=np.float32)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = R.iterate(st, trip, dtype=np.float32)
        ts.append(time.perf_counter() - t0)
    return {"ran": True, "what": "tests/hpf_restatement.py, dtype float32, one iteration (NumPy / "
            "SciPy, one thread of arithmetic)", "iteration_seconds": round(min(ts), 4),
            "iterations_seconds_all": [round(t, 4) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-ml25m", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--host-large", action="store_true")
    args = ap.parse_args()

    import scipy.sparse as sps
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

    ml = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
    ds = Dataset(ml.users, ml.items, ml._rows, ml._cols,
                 {"count": np.asarray(ml._attrs["rating"], np.float32) + np.float32(0.5)})
    legs = [("ml_latest_small", ds.interaction_matrix(field="count"), ds, True)]
    if not args.no_ml25m:
        from lkpy_amd import synth

        ratings = synth.ml25m_like()
        n_u, n_i = ratings.shape
        rows = np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr))
        big = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                      Vocabulary(np.arange(n_i), "item", reorder=False),
                      rows, ratings.indices, {"count": ratings.data.astype(np.float32)})
        legs.append(("ml25m_like", big.interaction_matrix(field="count"), big, args.host_large))
    failed = None
    for name, mat, dset, host in legs:
        mat = sps.csr_array(mat)
        mat.sort_indices()
        res[name], st = _device_leg(mat, args.iters, args.reps)
        emit()
        res[name]["train"] = _train_leg(dset, "count")
        emit()
        if args.no_torch:
            res[name]["torch_same_gpu"] = {"ran": False, "error": "not asked for (--no-torch)"}
        elif failed is not None:  # nothing more is started on a device after a failed leg
            res[name]["torch_same_gpu"] = {"ran": False,
                                           "error": f"not started: the {failed} leg failed"}
        else:
            res[name]["torch_same_gpu"] = _torch_leg(st, max(1, args.iters // 5))
            if not res[name]["torch_same_gpu"]["ran"]:
                failed = name
        del st
        torch.cuda.empty_cache()
        emit()
        res[name]["host_float32_restatement"] = _host_leg(mat, 3 if name == "ml_latest_small" else 1) \
            if host else {"ran": False, "error": "not asked for (--host-large): tens of GB of host "
                          "memory and about a minute per iteration"}
        emit()
    print(emit())


if __name__ == "__main__":
    main()
