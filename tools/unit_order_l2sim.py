#!/usr/bin/env python3
"""
CPU model of the L2 reuse of the long item rows' chunk launch: how many of the
rows of P that ``als_chunk_kernel`` gathers are still in the XCD's L2 when they are asked for,
under the row-major unit order and under the order ``lk_als_plan_order_units`` writes.

The matrix is ``lkpy_amd.synth.ml25m_like()`` as the engine holds it: users and items relabelled
longest first, an item row's entries by ascending ORIGINAL user (``make_plans_on_device``; with
``--sorted-rows`` by ascending new user, the host restatement's order).  The model:

* 8 XCDs, physical workgroup b on XCD b % 8, four units (one per wave) a workgroup;
* ``--resident`` (128) chunk workgroups resident per XCD, in launch order, a finished one
  replaced by the XCD's next; every resident wave gathers one 4-entry group per step;
* one LRU of P rows per XCD of ``--capacity`` (0.9) x 4 MiB, 256 B a row (padded k = 64).  The LRU
  is kept by step: a row is resident if fewer than the capacity of distinct rows were touched
  since the step of its last use.

With a device the ordered table is the plan's own (``ALSPlan.unit_table`` of the engine's item
plan); ``--host`` restates the relabelling and the order in NumPy and needs no device.

    python tools/unit_order_l2sim.py [--host] [--scale S] > profiles/unit_order_l2sim.txt
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

N_XCD = 8
ROW_BYTES = 256
L2_BYTES = 4 << 20


def simulate(beg, length, indices, resident=128, cap_rows=14745):
    "row-hit rate of one launch whose unit table (launch order) is (beg, length)"
    n = len(beg)
    n_wg = (n + 3) // 4
    end_all = beg + length
    hits = total = 0
    lane = np.arange(4)
    for x in range(N_XCD):
        queue = list(range(x, n_wg, N_XCD))[::-1]
        pos = np.zeros((resident, 4), np.int64)
        end = np.zeros((resident, 4), np.int64)

        def load(slot):
            b = queue.pop()
            u = np.arange(4 * b, min(4 * b + 4, n))
            pos[slot] = 0
            end[slot] = 0
            pos[slot, : len(u)] = beg[u]
            end[slot, : len(u)] = end_all[u]

        for s in range(resident):
            if queue:
                load(s)
        last = np.full(int(indices.max()) + 1, -1, np.int64)
        # cnt[t] = rows whose last use was step t (a step gathers at least one group of four)
        cnt = np.zeros(int(length.sum()) // 4 + len(length) + 2, np.int64)
        thr = 0  # rows last used at step >= thr are resident
        t = 0
        while True:
            live = pos < end
            if not live.any():
                break
            t += 1
            at = pos[live][:, None] + lane
            ok = at < end[live][:, None]
            rows = indices[at[ok]]
            total += len(rows)
            uniq = np.unique(rows)
            was = last[uniq]
            hit = was >= max(thr, 0)
            hit &= was >= 0
            hits += int(hit.sum()) + (len(rows) - len(uniq))
            old = was[was >= 0]
            if len(old):
                cnt[: t + 1] -= np.bincount(old, minlength=t + 1)
            cnt[t] = len(uniq)
            last[uniq] = t
            have, thr = 0, t
            while thr > 0 and have + cnt[thr] <= cap_rows:
                have += cnt[thr]
                thr -= 1
            thr += 1
            pos[live] += 4
            for s in np.flatnonzero(~(pos < end).any(axis=1)):
                if queue:
                    load(s)
    return hits / max(total, 1)


def deal(sorted_units, n):
    "launch position of each unit of the sorted list (lk_als_plan_order_units)"
    n_wg = (n + 3) // 4
    where = []
    for x in range(N_XCD):
        for b in range(x, n_wg, N_XCD):
            where.extend(range(4 * b, min(4 * b + 4, n)))
    table = np.empty(n, np.int64)
    table[np.asarray(where)] = sorted_units
    return table


def host_matrix(scale, sorted_rows):
    "(indptr, indices, key map) of the relabelled item rows, restated on the host"
    import scipy.sparse as sps

    from lkpy_amd import synth
    from lkpy_amd._als_engine import deal_rows

    ui = sps.csr_array(synth.ml25m_like(scale=scale))
    ulen, ilen = np.diff(ui.indptr), np.bincount(ui.indices, minlength=ui.shape[1])
    u_new, u_old, _ = deal_rows(ulen, 1)
    i_new, i_old, _ = deal_rows(ilen, 1)
    iu = sps.csr_array(ui.T)
    iu.sort_indices()  # an item's entries by ascending ORIGINAL user
    iu = iu[i_old]
    indices = u_new[iu.indices].astype(np.int32)
    indptr = iu.indptr.astype(np.int64)
    if sorted_rows:
        m = sps.csr_array((np.ones(len(indices), np.int8), indices, indptr),
                          shape=(len(i_old), len(u_old)))
        m.sort_indices()
        return indptr, m.indices.astype(np.int32), None
    return indptr, indices, u_old.astype(np.int64)


def row_major(indptr, unit, long_row=2048):
    lens = np.diff(indptr)
    beg, length = [], []
    for r in np.flatnonzero(lens > long_row):
        o = np.arange(0, lens[r], unit)
        beg.append(indptr[r] + o)
        length.append(np.minimum(unit, lens[r] - o))
    return np.concatenate(beg), np.concatenate(length)


def host_order(indptr, indices, key_map, beg, length):
    col = indices[beg]
    key = col if key_map is None else key_map[col]
    row = np.searchsorted(indptr, beg, side="right") - 1
    table = deal(np.lexsort((beg, row, key)), len(beg))
    return beg[table], length[table]


def device_tables(unit):
    "(indices, today's table, the plan's table) of the engine's item plan at this unit size"
    import torch

    from lkpy_amd import _native, synth
    from lkpy_amd._als_engine import HipBackend, ImplicitALSEngine

    os.environ["LK_ALS_REF_UNIT"] = str(unit)
    dev = torch.device("cuda:0")
    eng = ImplicitALSEngine(synth.ml25m_like(), 64, 0.1, 0.1, None, None,
                            HipBackend(64, dev, _native.SOLVER_AUTO))
    beg, length, _ = eng.i_plan.unit_table()
    indices = eng.i_plan.csr.indices.cpu().numpy()
    today = np.argsort(beg, kind="stable")  # row by row, a row's units one after the other
    return indices, (beg[today], length[today]), (beg, length)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host", action="store_true", help="no device: restate the order in NumPy")
    ap.add_argument("--sorted-rows", action="store_true",
                    help="(--host) rows list their entries by ascending NEW user")
    ap.add_argument("--scale", type=float, default=1.0, help="(--host) scale of the synthetic")
    ap.add_argument("--units", default="1024,512,256")
    ap.add_argument("--resident", type=int, default=128)
    ap.add_argument("--capacity", default="0.9,0.45", help="fractions of 4 MiB, comma separated")
    args = ap.parse_args()
    caps = [float(c) for c in args.capacity.split(",")]
    print(f"# unit_order_l2sim: resident {args.resident} workgroups / XCD, "
          f"{'host restatement' if args.host else 'plan tables from the device'}"
          f"{', rows sorted by new user' if args.sorted_rows else ''}, scale {args.scale}")
    print("# unit  capacity  order      units  row-hit-rate")
    if args.host:
        indptr, indices, key_map = host_matrix(args.scale, args.sorted_rows)
    for unit in (int(u) for u in args.units.split(",")):
        if args.host:
            today = row_major(indptr, unit)
            tables = [("row-major", today), ("ordered", host_order(indptr, indices, key_map, *today))]
            if key_map is not None:
                tables.append(("by-new-col", host_order(indptr, indices, None, *today)))
        else:
            indices, today, plan = device_tables(unit)
            tables = [("row-major", today), ("plan", plan)]
        for cap in caps:
            rows = int(cap * L2_BYTES / ROW_BYTES)
            for name, (beg, length) in tables:
                rate = simulate(beg, length, indices, args.resident, rows)
                print(f"{unit:6d}  {cap:8.2f}  {name:10s} {len(beg):6d}  {rate:.3f}", flush=True)


if __name__ == "__main__":
    main()
