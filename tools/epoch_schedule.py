#!/usr/bin/env python3
"""
The schedule of the LAST implicit-ALS epoch in a ``rocprofv3 --kernel-trace`` capture of the
headline workload (``rocprofv3 --kernel-trace --output-format csv -d DIR -o als -- python bench.py
--steps 5 --warmup 2``): one line per dispatch -- queue, workgroups, start and end in microseconds
from the epoch's first dispatch -- and the three statements of DESIGN.md section 4.1b about it.

    python tools/epoch_schedule.py DIR/als_kernel_trace.csv > profiles/<tag>_epoch_schedule.txt

(the committed tags: ``parent`` and ``change``).

An epoch ends with the Gramian of the new Q: the last epoch is what lies between the ends of the
third-last and the last ``gramian_finish_kernel`` (two per epoch).
"""
import csv
import re
import sys


def short(name: str) -> str:
    m = re.search(r"lk::(\w+)(<[^(]*>)?\(", name)
    if not m:
        return name[:60]
    return m.group(1) + (m.group(2) or "")


def main(path: str) -> int:
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            wg = max(int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1), 1)
            rows.append({
                "name": short(r["Kernel_Name"]), "queue": r.get("Queue_Id", "?"),
                "wgs": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) // wg,
                "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["t0"])
    fin = [r for r in rows if r["name"].startswith("gramian_finish_kernel")]
    if len(fin) < 3:
        print("fewer than three gramian_finish_kernel dispatches: no whole epoch in the trace")
        return 1
    lo, hi = fin[-3]["t1"], fin[-1]["t1"]
    ep = [r for r in rows if lo <= r["t0"] and r["t1"] <= hi]
    base = ep[0]["t0"]
    us = lambda t: (t - base) / 1e3  # noqa: E731
    queues = {q: n for n, q in enumerate(dict.fromkeys(r["queue"] for r in ep))}
    print(f"# last epoch of {path.split('/')[-1]}: {len(ep)} dispatches, "
          f"{us(hi):.1f} us from the first start to the last end; queue 0 = launch stream")
    print(f"{'queue':>5} {'wgs':>7} {'start_us':>9} {'end_us':>9}  kernel")
    for r in ep:
        print(f"{queues[r['queue']]:>5} {r['wgs']:>7} {us(r['t0']):>9.1f} {us(r['t1']):>9.1f}  "
              f"{r['name']}")

    # the three statements
    chunks = [r for r in ep if r["name"].startswith("als_chunk_kernel")]
    solves = [r for r in ep if r["name"].startswith("als_solve_kernel")]
    # als_solve_kernel<NT, IS64, EXPL, CTL, YREF, SEQY, ...>
    targs = lambda r: [a.strip() for a in r["name"][r["name"].index("<") + 1:-1].split(",")]  # noqa: E731
    long_ = [r for r in solves if targs(r)[4:6] == ["true", "false"]]   # YREF launches
    short_ = [r for r in solves if targs(r)[4:6] == ["false", "true"]]  # SEQY launches
    gfin = [r for r in ep if r["name"].startswith("gramian_finish_kernel")]
    print()
    if len(chunks) == 2 and len(long_) == 2 and len(short_) == 2 and len(gfin) == 2:
        cu, ci = chunks  # (user half first)
        print(f"item chunk starts {us(ci['t0']):.1f}, user half's gramian_finish ends "
              f"{us(gfin[0]['t1']):.1f}: chunk I starts before the Gramian tail ends: "
              f"{ci['t0'] < gfin[0]['t1']}")
        for half, lg, sh in zip("UI", long_, short_):
            print(f"half {half}: long-row solve ends {us(lg['t1']):.1f}, short-row solve ends "
                  f"{us(sh['t1']):.1f}: long rows done first: {lg['t1'] < sh['t1']}")
        su = short_[0]
        print(f"user chunk {us(cu['t0']):.1f} .. {us(cu['t1']):.1f}, user short-row solve "
              f"{us(su['t0']):.1f} .. {us(su['t1']):.1f}: they overlap: "
              f"{cu['t0'] < su['t1'] and su['t0'] < cu['t1']}")
    else:
        print(f"unexpected epoch shape: {len(chunks)} chunk, {len(long_)} long-row, "
              f"{len(short_)} short-row solve, {len(gfin)} gramian_finish dispatches")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
