#!/usr/bin/env python3
"""Pin the FA*IR thresholds and the greedy loop to the REFERENCE ITSELF, executed here.

The reference package does not import under this image's Python (make_als_fixtures.py), but
``lenskit/reranking/fair.py`` is plain NumPy / SciPy.  This script compiles single function
definitions of ``FAIRReranker`` *from the read-only checkout at run time* (``ast`` extraction:
nothing is copied into this repository) and commits only what they return:

* ``_compute_m_list``, ``_compute_blocks``, ``_compute_rejection_prob``,
  ``_binary_search_significance``: ``alpha_c`` and ``m_list`` for n in {1, 4, 10, 64, 65, 100,
  1000} x p in {0.1, 0.5, 0.9} x alpha in {1e-10, 0.1, 0.3};
* ``__call__``: it can be driven the same way, with a stand-in list object that answers
  ``len``, ``numbers`` and ``[positions]`` and a stand-in ``ItemList`` that hands the taken
  positions back -- its output positions for the lists of ``fair_restatement.golden_lists()``.

Run once where the reference checkout exists:

    python tests/golden/make_fair_fixtures.py

Output: ``tests/golden/fair_thresholds.json`` (data only).
"""
from __future__ import annotations

import __future__ as _future
import ast
import json
import sys
from collections import deque
from pathlib import Path
from types import SimpleNamespace

import numpy as np
from scipy.stats import binom

REF = Path("/root/reference")
SRC = REF / "src/lenskit/reranking/fair.py"
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
import fair_restatement as fr  # noqa: E402

NS = (1, 4, 10, 64, 65, 100, 1000)
PS = (0.1, 0.5, 0.9)
ALPHAS = (1e-10, 0.1, 0.3)


class _Log:
    def warning(self, *a, **k):
        pass


class _List:
    "what ``__call__`` asks of its input: a length, item numbers, a take by positions"

    def __init__(self, nums):
        self.nums = np.asarray(nums)

    def __len__(self):
        return len(self.nums)

    def numbers(self, vocabulary=None, missing=None):
        return self.nums

    def __getitem__(self, positions):
        return [int(x) for x in positions]


def _extract(name: str):
    "compile ONE method of FAIRReranker, annotations left unevaluated"
    tree = ast.parse(SRC.read_text())
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FAIRReranker").body
    fn = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.decorator_list = []
    mod = ast.Module(body=[fn], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "binom": binom, "deque": deque, "_log": _Log(),
          "ItemList": lambda taken, ordered=True: taken}
    code = compile(mod, f"<{SRC.relative_to(REF)}:{fn.lineno}>", "exec",
                   flags=_future.annotations.compiler_flag, dont_inherit=True)
    exec(code, ns)
    return ns[name], (fn.lineno, fn.end_lineno)


def main():
    fns, lines = {}, {}
    for name in ("_compute_m_list", "_compute_blocks", "_compute_rejection_prob",
                 "_binary_search_significance", "__call__"):
        fns[name], lines[name] = _extract(name)
    print("reference functions extracted at lines", lines)

    def model(n, p, alpha):
        me = SimpleNamespace(pmf_cache={}, config=SimpleNamespace(n=n, p=p, alpha=alpha))
        for name in ("_compute_m_list", "_compute_blocks", "_compute_rejection_prob",
                     "_binary_search_significance"):
            setattr(me, name, lambda *a, _f=fns[name], **k: _f(me, *a, **k))
        me.alpha_c = me._binary_search_significance(n=n, p=p, alpha=alpha)
        me.m_list = me._compute_m_list(n=n, p=p, alpha=me.alpha_c)
        return me

    grid = []
    for n in NS:
        for p in PS:
            for alpha in ALPHAS:
                me = model(n, p, alpha)
                grid.append({"n": n, "p": p, "alpha": alpha, "alpha_c": float(me.alpha_c),
                             "m_list": [int(x) for x in me.m_list]})
        print("n =", n, "done")

    lists = {}
    cache = {}
    for name, (flags, n, p, alpha, ask) in fr.golden_lists().items():
        key = (n, p, alpha)
        if key not in cache:
            cache[key] = model(n, p, alpha)
        me = cache[key]
        # item number = position; the last position's number is unknown (-1) where it is
        # unprotected, which the reference treats as unprotected too
        nums = np.arange(len(flags))
        if len(flags) and not flags[-1]:
            nums[-1] = -1
        me.protected_attributes = np.asarray(flags, dtype=bool)
        me.vocab = None
        taken = fns["__call__"](me, _List(nums), ask)
        lists[name] = {"flags": [int(f) for f in flags], "n": n, "p": p, "alpha": alpha,
                       "ask": ask, "positions": taken}
    with open(OUT / "fair_thresholds.json", "w") as f:
        json.dump({"lines": {k: list(v) for k, v in lines.items()}, "grid": grid,
                   "lists": lists}, f, separators=(",", ":"))
        f.write("\n")
    print("fair_thresholds.json:", len(grid), "grid points,", len(lists), "lists")


if __name__ == "__main__":
    main()
