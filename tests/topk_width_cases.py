"""
Inputs of ``tests/test_gpu_topk_widths.py``, built on the host so that
``tests/test_topk_stage1_host.py`` can check -- without a device -- that the restatement of
stage 1 predicts for each of them exactly the redo rows they were designed to have.

The small shape is the smallest at which every mechanism of the fused path is live: B = 130 rows
(two 128-row filter workgroups, the second with 2 live rows), I = 4099 items (17 tiles, the last
with 3 items), n = 10: stride 16, 257 sample columns (class 0 holds columns 0 and 256, every
other class one), and with the default item split 4 parts of 1024 candidates.
"""
from __future__ import annotations

import numpy as np

import topk_stage1_restatement as R

B0, I0, N0 = 130, 4099, 10
WIDTHS = [25, 32, 64, 100, 128, 200, 256]  # padded 32, 32, 64, 128, 128, 256, 256
VARIANTS = [("cmax", "wave"), ("panel", "sort"), ("cmax", "sort")]

# rows of the base block with a purpose
ROW_FREE, ROW_ZERO, ROW_FEW = 0, 1, 2  # no exclusions; all-zero user (overflow); < n items left
ROWS_ND = {3: 1, 4: 128, 5: 129, 6: 192, 7: 256}  # dirty classes, exactly
ROW_MESSY = 8  # unsorted, repeats, entries < 0 and >= I
ROWS_TIER2 = (9, 10)  # more than FUSED_LCAP, at most FUSED_CAP candidates
HOT = 1500  # items outside the sample that only the tier-2 rows see
# Knife-edge rows: their scores are feature 1 of the items alone, laid out so that the list holds
# n valid candidates ONLY at the threshold of the right rank -- one rank up (tau = 100) leaves 6
# candidates, one rank down (tau = 1) more than FUSED_CAP.  Sample columns 24, 32, .. 64 score 100,
# column 72 scores 10, every other sample column 1; five items outside the sample 50, 3000 of them 5.
ROW_KNIFE, ROW_KNIFE_128 = 11, 12  # no exclusions (rank r[0] = 7); columns 128 .. 255 excluded (r[128] = 6)
KNIFE_TOP, KNIFE_TAU = [16 * c for c in (24, 32, 40, 48, 56, 64)], 16 * 72
# larger calls (`expand`): base rows copied to both sides of a batch / range boundary
BATCH_OVERRIDES = {8190: ROWS_TIER2[0], 8191: ROW_FEW, 8192: ROW_FEW, 8193: ROWS_TIER2[1]}
OVERLAP_OVERRIDES = {65534: ROW_ZERO, 65535: ROWS_TIER2[0], 65536: ROWS_TIER2[1], 65537: ROW_FEW}


def designed(stage1: str, exact: bool = False):
    "(redo rows, undetermined rows) of the base block, by design"
    if exact:
        # every dirty class repaired: row 7 keeps class 0 alone, fewer than n: tau = -inf;
        # the knife-edge rows at rank n = 10: tau = 1, their lists overflow
        return [ROW_ZERO, ROW_FEW, 7, ROW_KNIFE, ROW_KNIFE_128], []
    if stage1.startswith("p"):
        # sample_tau_kernel strikes the exclusions out of the sample itself and keeps the rank:
        # row 7 keeps one sample column, fewer than r classes: tau = -inf, the list overflows;
        # row ROW_KNIFE_128 stays at rank 7: tau = 10, twelve candidates
        return [ROW_ZERO, ROW_FEW, 7], []
    # class maxima: ROW_KNIFE_128 drops 128 classes, rank 6: tau = 100, six candidates
    return [ROW_ZERO, ROW_FEW, ROW_KNIFE_128], [5, 6, 7]


def small_case(k: int, seed: int = 7) -> dict:
    rng = np.random.default_rng(seed + k)
    B, I, n = B0, I0, N0
    st = R.fused_stride(I, n)
    U = rng.standard_normal((B, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    # feature 0 belongs to the tier-2 rows: HOT items outside the sample score ~50 for them (more
    # than any sample item), so tau -- a rank of the sample -- lets all of them through
    U[:, 0] = 0.0
    hot = rng.choice(np.flatnonzero(np.arange(I) % st != 0), HOT, replace=False)
    Q[hot, 0] = 50.0
    for b in ROWS_TIER2:
        U[b] *= 0.05
        U[b, 0] = 1.0
    # feature 1 belongs to the knife-edge rows
    U[:, 1] = 0.0
    outside = np.flatnonzero(np.arange(I) % st != 0)
    Q[:, 1] = 1.0
    Q[outside, 1] = 0.0
    Q[rng.choice(outside, 3000, replace=False), 1] = 5.0
    Q[rng.random(I) < 0.05] = 0.0  # all-zero item rows
    Q[KNIFE_TOP, 1] = 100.0
    Q[KNIFE_TAU, 1] = 10.0
    Q[rng.choice(outside[(outside > 1000) & (outside < 2000)], 5, replace=False), 1] = 50.0
    Q[3000:3100] = Q[200:300]  # exact ties between distant tiles (0-1 / 11-12) and parts
    for b in (ROW_KNIFE, ROW_KNIFE_128):
        U[b] = 0.0
        U[b, 1] = 1.0
    U[ROW_ZERO] = 0.0
    lists = [rng.integers(0, I, int(l)) for l in rng.integers(1, 60, B)]  # any order, repeats
    lists[ROW_FREE] = np.zeros(0, np.int64)
    lists[ROW_ZERO] = np.zeros(0, np.int64)
    keep = rng.choice(I, 5, replace=False)
    lists[ROW_FEW] = rng.permutation(np.setdiff1d(np.arange(I), keep))
    for b, nd in ROWS_ND.items():
        cls = np.arange(256) if nd == 256 else rng.choice(256, nd, replace=False)
        lists[b] = rng.permutation(cls) * st  # sample columns 0 .. 255 only: column 256 stays
    lists[ROW_KNIFE] = np.zeros(0, np.int64)
    lists[ROW_KNIFE_128] = rng.permutation(np.arange(128, 256)) * st
    messy = np.concatenate([rng.integers(0, I, 40), [-1, -7, -st, I, I + 5, 2**31 - 1, -2**31,
                             st * R.fused_sample_items(I, n), 2**31 - st],  # (multiples of the stride too)
                            rng.integers(0, I, 40)])
    messy = np.concatenate([messy, messy[:25]])
    lists[ROW_MESSY] = rng.permutation(messy)
    lists[B - 1] = np.concatenate([lists[B - 1], [-3, I + 1], lists[B - 1][:3]])
    return dict(k=k, kp=R.padded_dim(k), B=B, I=I, n=n, U=U, Q=Q, lists=lists, hot=hot)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    ex = np.concatenate(lists).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, ex


def ordinary_rows(case) -> list:
    special = {ROW_FREE, ROW_ZERO, ROW_FEW, ROW_MESSY, ROW_KNIFE, ROW_KNIFE_128, *ROWS_ND, *ROWS_TIER2}
    return [b for b in range(case["B"]) if b not in special]


def expand(case, B: int, overrides: dict) -> dict:
    """
    A call of B rows over the same catalogue: rows 0 .. 129 are the base block, every later row
    is a copy (vector and exclusion list) of an ordinary base row, and ``overrides`` puts copies
    of chosen base rows at chosen places.  ``tmpl[b]`` = the base row that row b copies: its
    threshold and verdict are that row's.
    """
    tmpl = np.arange(B)
    ordinary = np.asarray(ordinary_rows(case))
    tmpl[case["B"]:] = ordinary[np.arange(B - case["B"]) % len(ordinary)]
    for b, t in overrides.items():
        tmpl[b] = t
    lists = [case["lists"][t] for t in tmpl]
    return dict(case, B=B, U=np.ascontiguousarray(case["U"][tmpl]), lists=lists, tmpl=tmpl, base=case)


def predict(oracle, case, **knobs) -> dict:
    "restatement over the distinct rows of the case; redo / undetermined / tier2 rows of the call"
    base = case.get("base", case)
    ptr, ex = csr(base["lists"])
    p = R.predict(lambda b: oracle.score_dense(base["Q"], base["U"][b]), base["U"], ptr, ex,
                  base["I"], case["n"], case["kp"], n_users=case["B"], **knobs)
    tmpl = case.get("tmpl", np.arange(case["B"]))
    for key in ("redo", "undetermined", "tier2"):
        p[key] = np.flatnonzero(np.isin(tmpl, p[key])).tolist()
    return p


def non_finite_case(k: int, seed: int = 11) -> dict:
    "the construction of test_score_topk_fused_non_finite_scores on the small catalogue"
    rng = np.random.default_rng(seed + k)
    B, I, n = B0, I0, N0
    U = rng.standard_normal((B, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.choice(I, 80, replace=False), 3] = np.nan  # NaN score for every user
    Q[rng.choice(I, 12, replace=False), 5] = np.inf  # +inf or -inf by the sign of U[:, 5]
    Q[::16][:50, 7] = np.inf  # many infinite scores inside the sample
    U[4] = 0.0
    U[4, 5] = 1.0  # inf * 0 = NaN elsewhere; +inf scores only
    U[B - 1, 5] = 2.0  # the last live row of the partial tile: the rows past it see +inf scores
    U[B - 1, 7] = 3.0  # too, and must write them nowhere
    return dict(k=k, kp=R.padded_dim(k), B=B, I=I, n=n, U=U, Q=Q,
                lists=[np.zeros(0, np.int64)] * B)


def n_edge_case(k: int, I: int, n: int, seed: int = 13) -> dict:
    rng = np.random.default_rng(seed + n + I)
    B = B0
    U = rng.standard_normal((B, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    lists = [rng.integers(0, I, int(l)) for l in rng.integers(0, 40, B)]
    lists[0] = np.zeros(0, np.int64)
    return dict(k=k, kp=R.padded_dim(k), B=B, I=I, n=n, U=U, Q=Q, lists=lists)
