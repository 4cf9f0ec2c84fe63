#!/usr/bin/env python3
"""
Timing driver of the FunkSVD trainer (csrc/funksvd.hip, ``lkpy_amd._device.funksvd_fit``).

    python tools/funksvd_time.py [--out FILE] [--reps N] [--no-big] [--variant-lib SO]

Two shapes, one feature each, shuffled with a fixed seed:

* ml-latest-small (tests/golden/ml_small.npz): the feature columns in LDS;
* the ML-25M-shaped synthetic of ``bench.py`` (``lkpy_amd.synth.ml25m_like``): the columns in
  global memory (``--no-big`` leaves it out).

For each: the plan's time (``lk_funksvd_plan_levels`` + ``lk_funksvd_plan_order``, host), its
depth and width histogram, the barriers the narrow-run walk removes, and the kernel's time per
epoch -- ``--reps`` launches of several epochs each, a host clock around launch and synchronise;
minimum, median and maximum.  Two yardsticks:

* the plain sequential host loop of tools/ub/funksvd_host_loop.cpp (``-O2``, built here with the
  C++ compiler if the shared object is missing), timed the same way on this machine's host, its
  column bits compared with the device's;
* ``--variant-lib``: a build of the library without the narrow-run walk
  (``python tools/build_variant.py nonarrow funksvd.hip -DLK_FUNKSVD_NARROW_RUNS=0``), timed in a
  child process of its own (``LK_AMD_LIBRARY``).
One JSON document.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LR, REG = 0.001, 0.015
HOST_SRC = ROOT / "tools" / "ub" / "funksvd_host_loop.cpp"
HOST_SO = ROOT / "tools" / "ub" / "funksvd_host_loop.so"
BINS = [1, 2, 8, 64, 256, 1024]  # width histogram: 1, 2, 3-8, 9-64, 65-256, 257-1024, above


def _samples(which):
    "(users, items, ratings, est, n_users, n_items), shuffled"
    if which == "ml_small":
        from lkpy_amd.data import load_movielens_npz

        ds = load_movielens_npz(ROOT / "tests" / "golden" / "ml_small.npz")
        rows, cols, vals = ds._rows, ds._cols, ds._attrs["rating"]
        shape = (ds.user_count, ds.item_count)
    else:
        from lkpy_amd import synth

        mat = synth.ml25m_like()
        rows = np.repeat(np.arange(mat.shape[0], dtype=np.int32), np.diff(mat.indptr))
        cols, vals, shape = mat.indices.astype(np.int32), mat.data.astype(np.float32), mat.shape
    shuf = np.arange(len(rows))
    np.random.default_rng(1).shuffle(shuf)
    ratings = np.ascontiguousarray(vals[shuf], dtype=np.float32)
    est = np.full(len(rows), np.float32(ratings.mean()), dtype=np.float32)
    return (np.ascontiguousarray(rows[shuf]), np.ascontiguousarray(cols[shuf]), ratings, est,
            *shape)


def _spread(per_epoch):
    s = sorted(per_epoch)
    return {"min": round(s[0], 7), "median": round(s[len(s) // 2], 7), "max": round(s[-1], 7)}


def _device_epochs(D, case, plan, epochs, reps):
    users, items, ratings, est, n_users, n_items = case
    args = (users, items, ratings, est, n_users, n_items, 1, epochs, LR, REG, 0.5, 5.0)
    D.funksvd_fit(*args, plan=plan)  # warm-up
    times, fit = [], None
    for _ in range(reps):
        stats = {}
        fit = D.funksvd_fit(*args, plan=plan, stats=stats)
        times.append(stats["train_seconds"] / epochs)
    return times, fit, stats["epochs_per_launch"]


def _host_loop():
    if not HOST_SO.exists():
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            return None
        subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o",
                               str(HOST_SO), str(HOST_SRC)])
    lib = ctypes.CDLL(str(HOST_SO))
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    lib.funksvd_host_epochs.restype = dbl
    lib.funksvd_host_epochs.argtypes = [vp, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int32,
                                        dbl, dbl, dbl, dbl, dbl]
    return lib


def _host_epochs(lib, case, epochs, reps):
    users, items, ratings, est, n_users, n_items = case
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    times = []
    for _ in range(reps):
        ucol = np.full(n_users, 0.1, np.float32)
        icol = np.full(n_items, 0.1, np.float32)
        t0 = time.perf_counter()
        lib.funksvd_host_epochs(hp(users), hp(items), hp(ratings), hp(est), len(users), hp(ucol),
                                hp(icol), epochs, LR, REG, 0.0, 0.5, 5.0)
        times.append((time.perf_counter() - t0) / epochs)
    return times, ucol, icol


def _schedule(plan, narrow):
    width = np.diff(plan.level_ptr)
    hist = np.bincount(np.searchsorted(BINS, width, side="left"), minlength=len(BINS) + 1)
    labels = ["1", "2", "3-8", "9-64", "65-256", "257-1024", "above 1024"]
    in_run = plan.run_end > np.arange(plan.depth)
    heads = in_run & np.concatenate([[True], plan.run_end[1:] != plan.run_end[:-1]])
    runs = int(heads.sum())  # (a run costs two barriers: behind its staging copy and at its end)
    return {"depth": plan.depth, "samples": int(plan.level_ptr[-1]),
            "width_max": int(width.max()), "width_mean": round(float(width.mean()), 1),
            "width_histogram": {labels[b]: int(c) for b, c in enumerate(hist)},
            "levels_in_narrow_runs": int(in_run.sum()), "narrow_runs": runs,
            "level_barriers_with_runs": int((~in_run).sum()) + 2 * runs,
            "level_barriers_without": plan.depth, "narrow_width": narrow}


def measure(which, epochs, reps, with_host):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    case = _samples(which)
    users, items, _, _, n_users, n_items = case
    plans = []
    for _ in range(3):
        t0 = time.perf_counter()
        plan = D.funksvd_plan(users, items, n_users, n_items)
        plans.append(time.perf_counter() - t0)
    in_lds = (n_users + n_items) * 4 <= D.funksvd_lds_column_bytes()
    res = {"shape": [n_users, n_items], "columns": "LDS" if in_lds else "global memory",
           "plan_seconds": _spread(plans),
           "schedule": _schedule(plan, int(_native.load().lk_funksvd_narrow_width()))}
    times, fit, per_launch = _device_epochs(D, case, plan, epochs, reps)
    res["device"] = {"epochs_per_launch": per_launch, "launches_timed": reps,
                     "seconds_per_epoch": _spread(times),
                     "samples_per_second": round(len(users) / sorted(times)[len(times) // 2])}
    if with_host:
        lib = _host_loop()
        if lib is None:
            res["host_loop"] = {"built": False}
        else:
            htimes, ucol, icol = _host_epochs(lib, case, epochs, reps)
            same = np.array_equal(ucol.view(np.uint32), fit[0][:, 0].copy().view(np.uint32)) and \
                np.array_equal(icol.view(np.uint32), fit[1][:, 0].copy().view(np.uint32))
            res["host_loop"] = {"built": True, "seconds_per_epoch": _spread(htimes),
                                "columns_bit_equal_to_device": bool(same),
                                "device_over_host": round(
                                    sorted(times)[len(times) // 2]
                                    / sorted(htimes)[len(htimes) // 2], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--child", action="store_true", help="device timings only, no host loop")
    args = ap.parse_args()

    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    res = {"device": torch.cuda.get_device_name(D.device()),
           "library": os.path.relpath(_native.LIB_PATH, ROOT),
           "lds_column_bytes": D.funksvd_lds_column_bytes(),
           "ml_small": measure("ml_small", 50, args.reps, not args.child)}
    if not args.no_big:
        res["ml25m_like"] = measure("ml25m_like", 2, max(3, args.reps // 2), not args.child)
    if args.variant_lib and not args.child:
        cmd = [sys.executable, __file__, "--child", "--reps", str(args.reps)]
        if args.no_big:
            cmd.append("--no-big")
        env = dict(os.environ, LK_AMD_LIBRARY=str(Path(args.variant_lib).resolve()))
        said = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout
        child = json.loads(said[said.index("{"):])
        res["without_narrow_runs"] = {"library": child["library"]}
        for key in ("ml_small", "ml25m_like"):
            if key in child:
                med = child[key]["device"]["seconds_per_epoch"]["median"]
                res["without_narrow_runs"][key] = {
                    "seconds_per_epoch": child[key]["device"]["seconds_per_epoch"],
                    "narrow_runs_over_variant": round(
                        res[key]["device"]["seconds_per_epoch"]["median"] / med, 3)}
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
