"""
NumPy restatement of what ``BiasedMFScorer.__call__`` computes around its row solve and its
``lk_score_dense`` row (src/lenskit/als/_common.py:133-175, _explicit.py:55-91,
basic/bias.py:166-241), written from explicit float32 / float64 casts only: it calls neither the
scorer nor ``BiasModel``.  The batched kernels (csrc/bmf_batch.hip) and the host composition are
both tested against it, bit for bit.

Three definitions:

``user_bias64``   ub = sum(uoff) / (count(finite uoff) + damping) in float64, NaN -> 0, with
                  uoff_j = (double)r_j - mu [- (double)b_i[j] for a known item].  ``np.sum`` of a
                  contiguous float64 array IS the order to reproduce (NumPy's pairwise sum).
``residuals``     the fold-in's CSR row: r_j - ((f32(mu) + b_i[j]) + f32(ub)) in float32, entries
                  with an unknown item or a non-finite rating dropped, the rest in ascending item
                  number (stable).
``finish``        the final score, rounded once to float32:
                    fold-in row   (double)dot + ((double)(f32(mu) + b_i) + ub)   in float64
                    stored row    dot + ((f32(mu) + b_i) + ub32)                  in float32
                    neither       NaN
"""
import numpy as np

INVALID, FOLD, STORED = 0, 1, 2  # a query's branch (include/lkamd.h: LK_BMF_*)


def user_bias64(ratings, item_nums, mu: float, item_biases, damping: float) -> np.float64:
    r = np.ascontiguousarray(ratings, dtype=np.float32)
    nums = np.asarray(item_nums)
    uoff = r.astype(np.float64) - np.float64(mu)
    known = nums >= 0
    uoff[known] = uoff[known] - np.asarray(item_biases, np.float32)[nums[known]].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ub = np.float64(np.sum(uoff)) / np.float64(np.count_nonzero(np.isfinite(uoff)) + damping)
    return np.float64(0.0) if np.isnan(ub) else np.float64(ub)


def item_part(item_nums, mu: float, item_biases) -> np.ndarray:
    "f32(mu) + b_i in float32; f32(mu) alone for an unknown item (-1)"
    nums = np.asarray(item_nums)
    out = np.full(len(nums), np.float32(mu), dtype=np.float32)
    known = nums >= 0
    out[known] = out[known] + np.asarray(item_biases, np.float32)[nums[known]]
    return out


def residuals(ratings, item_nums, mu: float, item_biases, damping: float):
    "-> (item numbers int32 ascending, residuals float32, ub float64)"
    r = np.ascontiguousarray(ratings, dtype=np.float32)
    nums = np.asarray(item_nums)
    ub = user_bias64(r, nums, mu, item_biases, damping)
    b = item_part(nums, mu, item_biases) + np.float32(ub)
    assert b.dtype == np.float32
    res = r - b
    keep = (nums >= 0) & np.isfinite(r)
    order = np.argsort(nums[keep], kind="stable")
    return nums[keep][order].astype(np.int32), res[keep][order].astype(np.float32), ub


def finish(dot, item_nums, mu: float, item_biases, mode: int, ub) -> np.ndarray:
    """float32 scores of one query: ``dot`` = the float32 entries of its lk_score_dense row at
    ``item_nums`` (-1: an unknown item -> NaN); ``ub``: float64 (fold-in) / float32 (stored)."""
    dot = np.ascontiguousarray(dot, dtype=np.float32)
    nums = np.asarray(item_nums)
    gb = item_part(nums, mu, item_biases)
    if mode == FOLD:
        out = (dot.astype(np.float64) + (gb.astype(np.float64) + np.float64(ub))).astype(np.float32)
    elif mode == STORED:
        out = dot + (gb + np.float32(ub))
        assert out.dtype == np.float32
    else:
        out = np.full(len(nums), np.nan, dtype=np.float32)
    out = out.copy()
    out[nums < 0] = np.nan
    return out


def bits(a) -> np.ndarray:
    "float32 bit patterns, every NaN the same"
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
