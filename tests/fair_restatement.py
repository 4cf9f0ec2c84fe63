"""
FA*IR (Zehlike et al. 2017) restated in plain NumPy / SciPy, the yardstick of tests/test_fair_host.py
and tests/test_gpu_fair.py: the thresholds, the adjusted significance, and the greedy loop on plain
arrays with a record of what happened on the way (which queue ran dry, whether the list moved).

Written from the paper's Algorithms 1 and 2 and the semantics of ``lenskit.reranking.fair`` (same
SciPy calls, so the thresholds agree exactly); tests/golden/fair_thresholds.json pins it to the
reference's own functions.  All list results are integers or copied float bits: comparisons against
it are exact.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.stats import binom


def thresholds(n: int, p: float, alpha: float) -> np.ndarray:
    "m[i] for prefixes of 1..n items: the alpha-quantile of Bin(i + 1, p), kept inside 0..i+1"
    q = binom.ppf(alpha, np.arange(1, n + 1), p)  # (one call for all prefixes, as the reference)
    return np.asarray([int(min(max(q[i], 0), i + 1)) for i in range(n)], dtype=np.int64)


def blocks(m) -> list[int]:
    "lengths of the runs that end where m steps up"
    if len(m) == 0 or m[-1] == 0:
        return []
    ends = [i + 1 for i in range(len(m)) if m[i] != (m[i - 1] if i else 0)]
    return [e - (ends[k - 1] if k else 0) for k, e in enumerate(ends)]


def fail_probability(n: int, p: float, alpha_c: float) -> float:
    "P(a ranking with iid Bernoulli(p) flags misses some threshold of thresholds(n, p, alpha_c))"
    dist = np.array([1.0])
    for j, b in enumerate(blocks(thresholds(n, p, alpha_c)), start=1):
        dist = np.convolve(binom.pmf(np.arange(b + 1), b, p), dist)
        dist[j - 1] = 0.0
    return float(1 - dist.sum())


def adjusted_alpha(n: int, p: float, alpha: float) -> float:
    lo, hi = 0, 1
    for _ in range(100):
        mid = (lo + hi) / 2
        f = fail_probability(n, p, mid)
        if f > alpha:
            hi = mid
        else:
            lo = mid
        if abs(f - alpha) < 1e-10 or hi - lo < 1e-10:
            break
    return (lo + hi) / 2


@dataclass
class Trace:
    positions: np.ndarray  # the input position each output slot takes
    p_dry_short: bool  # some slot had c < m[i] with no protected item left
    u_dry: bool  # some slot found no unprotected item left
    constrained: bool  # neither of the above: the prefix constraints must hold


def rerank_flags(flags, m, n: int) -> Trace:
    "the greedy loop on one list's flags (bool, list order)"
    flags = np.asarray(flags, dtype=bool)
    prot = [j for j in range(len(flags)) if flags[j]]
    rest = [j for j in range(len(flags)) if not flags[j]]
    a = b = c = 0  # heads of prot / rest, protected count
    out = []
    p_short = u_dry = False
    for i in range(min(n, len(flags))):
        have_p, have_u = a < len(prot), b < len(rest)
        if c < m[i] and not have_p:
            p_short = True
        if not have_u:
            u_dry = True
        if have_p and (c < m[i] or not have_u or prot[a] < rest[b]):
            out.append(prot[a])
            a += 1
            c += 1
        else:
            out.append(rest[b])
            b += 1
    return Trace(np.asarray(out, dtype=np.int64), p_short, u_dry, not (p_short or u_dry))


def row_length(row, length=None) -> int:
    "a row's length: given, or up to its first negative entry"
    if length is not None:
        return int(min(max(length, 0), len(row)))
    neg = np.flatnonzero(np.asarray(row) < 0)
    return int(neg[0]) if len(neg) else len(row)


def item_flags(items, table) -> np.ndarray:
    "flags of item numbers; numbers outside the table are unprotected"
    items = np.asarray(items, dtype=np.int64)
    ok = (items >= 0) & (items < len(table))
    out = np.zeros(len(items), dtype=bool)
    out[ok] = np.asarray(table, dtype=bool)[items[ok]]
    return out


def rerank_rows(lists, table, m, n: int, *, lengths=None, scores=None):
    """
    Every row of ``lists`` [B x L] reranked: (items int32 [B x n] with -1 padding, scores float32
    [B x n] with NaN padding or None, positions int32 [B x n] with -1 padding, the rows' traces).
    """
    lists = np.asarray(lists, dtype=np.int32)
    B = lists.shape[0]
    items = np.full((B, n), -1, dtype=np.int32)
    pos = np.full((B, n), -1, dtype=np.int32)
    sc = None if scores is None else np.full((B, n), np.nan, dtype=np.float32)
    traces = []
    for r in range(B):
        ln = row_length(lists[r], None if lengths is None else lengths[r])
        t = rerank_flags(item_flags(lists[r, :ln], table), m, n)
        k = len(t.positions)
        items[r, :k] = lists[r, t.positions]
        pos[r, :k] = t.positions
        if sc is not None:
            sc[r, :k] = np.asarray(scores, dtype=np.float32)[r, t.positions]
        traces.append(t)
    return items, sc, pos, traces


# ---- the lists whose reference output tests/golden/fair_thresholds.json records -----------------

def _mix(x: int) -> int:
    x = (x ^ (x >> 16)) * 0x45D9F3B & 0xFFFFFFFF
    x = (x ^ (x >> 16)) * 0x45D9F3B & 0xFFFFFFFF
    return x ^ (x >> 16)


def hashed_flags(length: int, share: float, salt: int) -> np.ndarray:
    "flags from an integer hash (no RNG stream): position j is protected at about ``share``"
    return np.asarray([_mix(j * 2654435761 + salt * 40503 + 17) % 10000 < share * 10000
                       for j in range(length)], dtype=bool)


def golden_lists():
    "name -> (flags in list order, config n, p, alpha, requested n or None)"
    out = {
        "paper-example": (np.isin(np.arange(10), [6, 8]), 10, 0.5, 0.1, None),
        "none-protected": (np.zeros(30, dtype=bool), 10, 0.5, 0.1, None),
        "all-protected": (np.ones(30, dtype=bool), 10, 0.5, 0.1, None),
        "last-only": (np.arange(40) == 39, 10, 0.5, 0.1, None),
        "short-list": (hashed_flags(7, 0.3, 1), 10, 0.5, 0.1, None),
        "smaller-n": (hashed_flags(50, 0.2, 2), 10, 0.5, 0.1, 6),
    }
    for share in (0.05, 0.2, 0.5):
        for L in (100, 400):
            out[f"hash-{share}-{L}"] = (hashed_flags(L, share, L), 100, 0.5, 0.1, None)
    out["p09-tight"] = (hashed_flags(300, 0.3, 5), 64, 0.9, 0.3, None)
    out["p09-loose"] = (hashed_flags(300, 0.3, 6), 64, 0.9, 1e-10, None)
    return out
