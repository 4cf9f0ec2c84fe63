"""
Stage 1 of the fused top-N path (``csrc/topk.hip``) restated in NumPy, and from its threshold the
REDO VERDICT of a row: which rows the device must list for the exact redo, and no others.

Not a second implementation of the path -- nothing here selects or sorts.  It answers one question
per row, from the row's exact scores (``oracle.score_dense``: the kernels' k-ordered fmaf chain,
the same bits): what is ``tau``, and does the row end without ``n`` valid candidates?

The knobs the library reads from the environment are arguments here (``div`` = LK_TOPK_SAMPLE_DIV,
``exact`` = LK_TOPK_TAU_EXACT, ``stage1`` = LK_TOPK_STAGE1, ``split`` = LK_TOPK_SPLIT,
``fused_rows`` = LK_TOPK_FUSED_ROWS, ``overlap`` = LK_TOPK_OVERLAP).
"""
from __future__ import annotations

import numpy as np

SC_UB, SC_IB, SC_KC = 64, 256, 32
SAMPLE_DIV_DEFAULT = 24
FUSED_CAP = 2048  # candidates per row
FUSED_MAX_N = 128
FUSED_REDO_CAP = 4096
FUSED_LCAP = 1024  # candidates the first selection tier holds (both first-tier kernels)
CMAX_LDS_EXTRA = 16 + 256 + 256
CMAX_DROP_MAX = 128
CMAX_REPAIR_MAX = 64
CMAX_RANKS = 256 - CMAX_REPAIR_MAX + 1

UNDETERMINED = None  # tau of a row whose repaired classes depend on the order of LDS atomics


# ---- sample geometry -------------------------------------------------------------------------
def fused_sub_items(n_items: int, n: int, div: int = 0) -> int:
    d = div if 2 <= div <= 64 else SAMPLE_DIV_DEFAULT
    s = n_items // d
    s = max(s, 16 * n)
    s = (s + 255) // 256 * 256
    return s if s < n_items else n_items


def fused_stride(n_items: int, n: int, div: int = 0) -> int:
    return max(1, n_items // fused_sub_items(n_items, n, div))


def fused_sample_items(n_items: int, n: int, div: int = 0) -> int:
    st = fused_stride(n_items, n, div)
    return (n_items + st - 1) // st


def fused_tau_rank(n_items: int, n: int, keep: float = 1.0, exact: bool = False, div: int = 0) -> int:
    "smallest r >= 1 with P[Binomial(n - 1, keep * sample / catalogue) >= r] <= 1e-6, else n"
    if exact:
        return n
    f64 = np.float64
    with np.errstate(all="ignore"):  # f = 1: 0 / 0, as in the C (the NaN tail never passes: r = n)
        f = f64(keep) * f64(fused_sample_items(n_items, n, div)) / f64(n_items)
        m = n - 1
        pmf = f64(1.0)
        for _ in range(m):
            pmf = pmf * (f64(1.0) - f)
        cdf = f64(0.0)
        for r in range(m + 1):
            if r >= 1 and f64(1.0) - cdf <= 1.0e-6:
                return r
            cdf = cdf + pmf
            pmf = pmf * f64(m - r) / f64(r + 1) * f / (f64(1.0) - f)
    return n


def padded_dim(k: int) -> int:
    "lk_padded_dim for k <= 1024"
    for p in (16, 32, 64, 128, 256):
        if k <= p:
            return p
    return (k + 63) // 64 * 64


def use_fused(n_users: int, n_items: int, n: int, kp: int, min_users: int = 8192,
              min_items: int = 16384) -> bool:
    return (1 <= n <= FUSED_MAX_N and n_items >= min_items and n_items >= 64 * n
            and n_users >= min_users and kp % SC_KC == 0 and kp <= 256)


def cmax_usable(n_items: int, n: int, stage1: str = "cmax", div: int = 0) -> bool:
    words = (fused_sample_items(n_items, n, div) + 31) // 32
    return not stage1.startswith("p") and (words + CMAX_LDS_EXTRA) * 16 <= 65536


def fused_rows(n_items: int, n: int, stage1: str = "cmax", div: int = 0, env_rows: int | None = None) -> int:
    "rows per fused batch"
    nsub = (fused_sample_items(n_items, n, div) + 63) // 64 * 64
    panel = not cmax_usable(n_items, n, stage1, div)
    r = 262144 if env_rows is None else env_rows
    by_panel = (16 << 30) // (nsub * 4) if panel else r
    r = min(r, by_panel)
    r = r // 128 * 128
    if r > 65536:
        r = r // 65536 * 65536
    lo = min(8192, by_panel // 128 * 128)
    lo = max(lo, 128)
    return max(r, lo)


def filter_parts(rows: int, n_items: int, kp: int, split: bool = True) -> int:
    wgs = (rows + 2 * SC_UB - 1) // (2 * SC_UB)
    n_itiles = (n_items + SC_IB - 1) // SC_IB
    if kp not in (32, 64, 128, 256) or not split or wgs >= 512 or n_itiles < 8:
        return 1
    parts = min(512 // wgs, n_itiles // 4, 64)
    return 1 if parts < 2 else parts


def filter_part_cap(parts: int) -> int:
    if parts < 2:
        return FUSED_CAP
    c = (2 * FUSED_CAP // parts + 127) // 128 * 128
    return min(max(c, 512), FUSED_CAP)


def geometry(n_users: int, n_items: int, n: int, kp: int, *, stage1: str = "cmax", div: int = 0,
             split: bool = True, env_rows: int | None = None, overlap: bool = True,
             exact: bool = False) -> dict:
    "what lk_score_topk_last_report says of a fused call before any row is looked at"
    fr = fused_rows(n_items, n, stage1, div, env_rows)
    batches = (n_users + fr - 1) // fr
    parts = filter_parts(min(n_users, fr), n_items, kp, split) if batches == 1 else 1
    used = False
    for b in range(batches):
        rows = min(fr, n_users - b * fr)
        wgs = (rows + 127) // 128
        used = used or (overlap and wgs > 512 and wgs % 512 != 0)
    return dict(batches=batches, parts=parts, part_cap=filter_part_cap(parts), overlap=used,
                stride=fused_stride(n_items, n, div), n_sample=fused_sample_items(n_items, n, div),
                r_tau=fused_tau_rank(n_items, n, 1.0, exact, div),
                cmax=cmax_usable(n_items, n, stage1, div), rows_per_batch=fr)


# ---- thresholds ------------------------------------------------------------------------------
def _excluded_sample_columns(excl, stride: int, n_sub: int) -> np.ndarray:
    e = np.asarray(excl, dtype=np.int64)
    e = e[(e >= 0) & (e % stride == 0)]
    j = e // stride
    return np.unique(j[j < n_sub])


def _rth_largest(vals: np.ndarray, r: int) -> float:
    "r-th largest of the valid (non-NaN) class values; fewer than r of them: -inf"
    v = vals[~np.isnan(vals)]
    if len(v) < r:
        return -np.inf
    return float(np.sort(v)[::-1][r - 1])


def _class_max(sample: np.ndarray, cls: np.ndarray, n_cls: int = 256) -> np.ndarray:
    out = np.full(n_cls, np.nan, np.float32)
    np.fmax.at(out, cls, sample)  # fmax: NaN is "nothing yet" on either side
    return out


def tau_panel(scores: np.ndarray, excl, n_items: int, n: int, *, exact: bool = False, div: int = 0):
    """
    ``sample_tau_kernel``: the sample row is swept as float4s, float4 i belongs to class i mod 256
    (the tail columns past the last whole float4 to classes 0, 1, 2); excluded and NaN columns are
    skipped; tau = the r-th largest CLASS maximum, r = fused_tau_rank of the whole sample whatever
    the exclusions.  Returns (tau, 0).
    """
    st, n_sub = fused_stride(n_items, n, div), fused_sample_items(n_items, n, div)
    sample = np.array(scores[::st][:n_sub], dtype=np.float32)
    assert len(sample) == n_sub
    sample[_excluded_sample_columns(excl, st, n_sub)] = np.nan
    j = np.arange(n_sub)
    n4 = n_sub // 4
    cls = np.where(j < 4 * n4, (j // 4) % 256, j - 4 * n4)
    return _rth_largest(_class_max(sample, cls), fused_tau_rank(n_items, n, 1.0, exact, div)), 0


def tau_cmax(scores: np.ndarray, excl, n_items: int, n: int, *, exact: bool = False, div: int = 0):
    """
    ``sample_cmax_kernel`` + ``cmax_tau_kernel``: 256 class maxima over the sample columns
    j = c (mod 256), NaN skipped, taken WITHOUT the exclusions; classes holding an excluded sample
    column are dirty.  nd <= drop_max dirty classes: dropped, rank r[nd].  More: min(nd, repair_max)
    are repaired (maximum over their un-excluded columns), the rest dropped, rank
    r[nd - repaired] -- WHICH ones is the order of LDS atomics unless all are repaired.
    Returns (tau or UNDETERMINED, nd).
    """
    st, n_sub = fused_stride(n_items, n, div), fused_sample_items(n_items, n, div)
    sample = np.array(scores[::st][:n_sub], dtype=np.float32)
    assert len(sample) == n_sub
    j = np.arange(n_sub)
    cmax = _class_max(sample, j % 256)
    ranks = [fused_tau_rank(n_items, n, (256 - d) / 256.0, exact, div) for d in range(CMAX_RANKS)]
    drop_max = 0 if exact else CMAX_DROP_MAX
    repair_max = 256 if exact else CMAX_REPAIR_MAX
    ex = _excluded_sample_columns(excl, st, n_sub)
    dirty = np.unique(ex % 256)
    nd = len(dirty)
    if nd == 0:
        return _rth_largest(cmax, ranks[0]), 0
    if nd <= drop_max:
        cmax[dirty] = np.nan
        return _rth_largest(cmax, ranks[nd]), nd
    n_rep = min(nd, repair_max)
    if n_rep < nd:
        return UNDETERMINED, nd
    clean = sample.copy()
    clean[ex] = np.nan
    rep = _class_max(clean, j % 256)
    cmax[dirty] = rep[dirty]
    return _rth_largest(cmax, ranks[nd - n_rep]), nd


def stage1_tau(scores, excl, n_items, n, *, stage1="cmax", exact=False, div=0):
    if cmax_usable(n_items, n, stage1, div):
        return tau_cmax(scores, excl, n_items, n, exact=exact, div=div)
    return tau_panel(scores, excl, n_items, n, exact=exact, div=div)


# ---- the redo verdict -------------------------------------------------------------------------
def row_verdict(scores: np.ndarray, excl, n: int, tau, parts: int = 1) -> dict:
    """
    Stage 2 appends every item whose score is not NaN and >= tau, excluded or not: part p of a
    split launch walks the item tiles p, p + parts, ... into a sub-list of filter_part_cap(parts)
    entries.  A row is redone iff a sub-list overflows, the whole list holds more than FUSED_CAP,
    or fewer than n of the candidates are un-excluded.  ``redo`` is None when tau is undetermined
    and the verdict depends on it.
    """
    scores = np.asarray(scores, dtype=np.float32)
    n_items = len(scores)
    e = np.asarray(excl, dtype=np.int64)
    e = e[(e >= 0) & (e < n_items)]
    free = np.ones(n_items, bool)
    free[e] = False
    if int((free & ~np.isnan(scores)).sum()) < n:  # whatever tau is
        return dict(redo=True, why="fewer than n valid items", count=None, valid=None, tier2=None)
    if tau is UNDETERMINED:
        return dict(redo=None, why="undetermined", count=None, valid=None, tier2=None)
    with np.errstate(invalid="ignore"):
        hit = scores >= np.float32(tau)  # NaN fails
    count = int(hit.sum())
    per_part = np.bincount((np.arange(n_items) // SC_IB) % parts, weights=hit, minlength=parts)
    valid = int((hit & free).sum())
    if parts > 1 and per_part.max() > filter_part_cap(parts):
        why = "a part overflows"
    elif count > FUSED_CAP:
        why = "list overflows"
    elif valid < n:
        why = "threshold too high"
    else:
        why = None
    return dict(redo=why is not None, why=why, count=count, valid=valid,
                tier2=why is None and count > FUSED_LCAP)


def predict(score_row, users, excl_ptr, excl_items, n_items: int, n: int, kp: int, *, stage1="cmax",
            exact=False, div=0, split=True, env_rows=None, overlap=True, rows=None,
            n_users=None) -> dict:
    """
    The redo set of a whole call: ``score_row(b)`` gives row b's exact scores.  Returns the
    geometry, the rows that must be redone, the undetermined rows, per-row candidate counts and
    dirty-class counts (``rows``: look at these rows only; ``n_users``: the call has this many
    rows -- the geometry is the call's -- of which ``users`` are the distinct ones).
    """
    B = len(users) if n_users is None else n_users
    geo = geometry(B, n_items, n, kp, stage1=stage1, div=div, split=split, env_rows=env_rows,
                   overlap=overlap, exact=exact)
    redo, und, counts, nds, tier2 = [], [], {}, {}, []
    for b in (range(len(users)) if rows is None else rows):
        s = score_row(b)
        ex = excl_items[excl_ptr[b]:excl_ptr[b + 1]] if excl_ptr is not None else np.zeros(0, np.int64)
        tau, nd = stage1_tau(s, ex, n_items, n, stage1=stage1, exact=exact, div=div)
        v = row_verdict(s, ex, n, tau, geo["parts"])
        nds[b] = nd
        counts[b] = v["count"]
        if v["redo"] is None:
            und.append(b)
        elif v["redo"]:
            redo.append(b)
        elif v["tier2"]:
            tier2.append(b)
    return dict(geometry=geo, redo=redo, undetermined=und, counts=counts, nd=nds, tier2=tier2)
