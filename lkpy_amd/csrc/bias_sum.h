// bias_sum.h -- the user-offset sum of `BiasModel.compute_for_items` (src/lenskit/basic/bias.py:
// 166-240) in NumPy's own order, for every kernel that derives a user bias from training ratings
// (predict_merge.hip: lk_bias_user_offsets; bmf_batch.hip: lk_bmf_residual_rows).
//
// The sum is NumPy's `np.sum` of a contiguous float64 array, whose order is fixed (pairwise_sum in
// NumPy's loops_utils): blocks of 8192 elements added in sequence from 0.0; inside a block, n < 8:
// a sequential sum from 0.0; n <= 128: eight accumulators started at a[0..7], stepped by eight up
// to n - n % 8, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the tail added in
// sequence; larger n: split at n2 = n / 2 - (n / 2) % 8 and the halves' sums added.  The accumulate
// type (`uoff_t`) and that order live in `uoff`, `leaf_sum`, `block_sum` and `row_user_bias` below
// and nowhere else.
#pragma once

#include "common.h"

// The host sums are plain adds and one divide; nothing may be fused.
#pragma clang fp contract(off)

namespace lk {
namespace {

// The type the host computes `uoff` and its sum in (float64: `np.asarray(ratings, np.float64)`).
using uoff_t = double;

constexpr int PM_BLOCK = 8192;  // NumPy's reduction buffer: block sums are added in sequence
constexpr int PM_LEAF = 128;    // pairwise_sum's PW_BLOCKSIZE
constexpr int PM_NODES = 160;   // split-tree nodes of one block: 129 at most for n <= 8192

struct UoffSrc {
    const int32_t *indices;
    const float *values;
    const float *item_biases;  // NULL: no item term
    int64_t n_items;
    uoff_t global_bias;
};

// uoff_j = r_j - mu, minus b_i where the model has item biases (basic.py: `uoff[rm] -= ...`)
__device__ __forceinline__ uoff_t uoff(const UoffSrc &src, int64_t e)
{
    uoff_t v = (uoff_t)src.values[e] - src.global_bias;
    if (src.item_biases) {
        const int32_t c = src.indices[e];
        if (c >= 0 && c < src.n_items) v = v - (uoff_t)src.item_biases[c];
    }
    return v;
}

// pairwise_sum for n <= 128 (one leaf of the split tree), elements [lo, lo + n)
__device__ uoff_t leaf_sum(const UoffSrc &src, int64_t lo, int n)
{
    if (n < 8) {
        uoff_t res = 0.0;
        for (int i = 0; i < n; ++i) res = res + uoff(src, lo + i);
        return res;
    }
    uoff_t r0 = uoff(src, lo + 0), r1 = uoff(src, lo + 1), r2 = uoff(src, lo + 2),
           r3 = uoff(src, lo + 3), r4 = uoff(src, lo + 4), r5 = uoff(src, lo + 5),
           r6 = uoff(src, lo + 6), r7 = uoff(src, lo + 7);
    const int m = n - n % 8;
    for (int i = 8; i < m; i += 8) {
        r0 = r0 + uoff(src, lo + i + 0);
        r1 = r1 + uoff(src, lo + i + 1);
        r2 = r2 + uoff(src, lo + i + 2);
        r3 = r3 + uoff(src, lo + i + 3);
        r4 = r4 + uoff(src, lo + i + 4);
        r5 = r5 + uoff(src, lo + i + 5);
        r6 = r6 + uoff(src, lo + i + 6);
        r7 = r7 + uoff(src, lo + i + 7);
    }
    uoff_t res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int i = m; i < n; ++i) res = res + uoff(src, lo + i);
    return res;
}

struct BlockTree {
    int lo[PM_NODES];
    int n[PM_NODES];
    int child[PM_NODES];  // first child (the second follows it), -1 for a leaf
    uoff_t val[PM_NODES];
    int count;
};

// pairwise_sum of one block (n <= 8192) starting at element `base`; the value is lane 0's.  The
// split tree is laid out breadth first in LDS (children after their parent), the leaves are
// summed by the lanes in parallel, and lane 0 adds the siblings back to front -- the recursion's
// arithmetic without a call stack.
__device__ uoff_t block_sum(const UoffSrc &src, int64_t base, int n, BlockTree &t)
{
    const int lane = threadIdx.x;
    if (n <= PM_LEAF) return lane == 0 ? leaf_sum(src, base, n) : 0.0;
    __syncthreads();  // (the previous block's tree is no longer read)
    if (lane == 0) {
        int cnt = 1;
        t.lo[0] = 0;
        t.n[0] = n;
        for (int i = 0; i < cnt; ++i) {
            const int m = t.n[i];
            if (m > PM_LEAF) {
                int n2 = m / 2;
                n2 -= n2 % 8;
                t.lo[cnt] = t.lo[i];
                t.n[cnt] = n2;
                t.lo[cnt + 1] = t.lo[i] + n2;
                t.n[cnt + 1] = m - n2;
                t.child[i] = cnt;
                cnt += 2;
            } else {
                t.child[i] = -1;
            }
        }
        t.count = cnt;
    }
    __syncthreads();
    const int cnt = t.count;
    for (int i = lane; i < cnt; i += WAVE)
        if (t.child[i] < 0) t.val[i] = leaf_sum(src, base + t.lo[i], t.n[i]);
    __syncthreads();
    uoff_t res = 0.0;
    if (lane == 0) {
        for (int i = cnt - 1; i >= 0; --i) {
            const int c = t.child[i];
            if (c >= 0) t.val[i] = t.val[c] + t.val[c + 1];
        }
        res = t.val[0];
    }
    return res;
}

// ub = sum(uoff) / (count(finite uoff) + damping), NaN -> 0, of the n entries from `s` on, as a
// float64 (the host rounds it to float32 where it adds it to float32 scores): the value is lane
// 0's.  Called by every lane of a one-wave block.
__device__ double row_user_bias(const UoffSrc &src, int64_t s, int64_t n, double damping,
                                BlockTree &tree)
{
    const int lane = threadIdx.x;
    int cnt = 0;  // np.sum(np.isfinite(uoff)): any order (a row holds < 2^31 entries)
    for (int64_t i = lane; i < n; i += WAVE) cnt += __builtin_isfinite(uoff(src, s + i)) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
    uoff_t total = 0.0;
    for (int64_t b = 0; b < n; b += PM_BLOCK) {
        const int m = (int)(n - b < PM_BLOCK ? n - b : PM_BLOCK);
        const uoff_t bs = block_sum(src, s + b, m, tree);
        total = total + bs;
    }
    double ub = (double)total / ((double)cnt + damping);
    if (__builtin_isnan(ub)) ub = 0.0;
    return ub;
}

}  // namespace
}  // namespace lk
