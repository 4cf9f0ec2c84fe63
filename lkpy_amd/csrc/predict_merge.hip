// predict_merge.hip -- the rating-predictor tail of std:topn-predict for a BATCH of queries, gfx950.
//
// `batch.predict` over the iknn-explicit pipeline scores every (query, target) pair with
// lk_iknn_score_batch; what the reference then does per query on the host is here:
//
//   bias_user_offsets_kernel  the user bias `BiasModel.compute_for_items` derives from the
//                             query's training ratings (src/lenskit/basic/bias.py:166-240):
//                             ub = sum(uoff) / (count(finite uoff) + damping), NaN -> 0,
//                             uoff = r - mu [- b_i].  One wave per query; the row is read
//                             straight from the training matrix by user number.
//   predict_merge_kernel      the item mean added back to the kNN score (src/lenskit/knn/
//                             item.py:282) and `FallbackScorer` (src/lenskit/basic/composite.py):
//                             a NaN score becomes mu + b_i + ub with is_fallback set.  One thread
//                             per (query, target) entry.
//
// Both follow the host mirror (lkpy_amd/basic.py, knn.py) operation for operation, so the lists
// are the per-query composition's bit for bit.  The user-bias sum is NumPy's `np.sum` of a
// contiguous float64 array, whose order is fixed (pairwise_sum in NumPy's loops_utils): blocks of
// 8192 elements added in sequence from 0.0; inside a block, n < 8: a sequential sum from 0.0;
// n <= 128: eight accumulators started at a[0..7], stepped by eight up to n - n % 8, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the tail added in sequence; larger n: split
// at n2 = n / 2 - (n / 2) % 8 and the halves' sums added.  The accumulate type (`uoff_t`) and that
// order live in `uoff`, `leaf_sum` and `block_sum` below and nowhere else.
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

template <typename IT>
__global__ __launch_bounds__(WAVE) void bias_user_offsets_kernel(
    const IT *__restrict__ indptr, UoffSrc src, int64_t n_users, int64_t n_queries,
    const int32_t *__restrict__ user_nums, double damping, float *__restrict__ out_ub,
    uint8_t *__restrict__ out_add)
{
    __shared__ BlockTree tree;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= n_queries) return;
    const int32_t u = user_nums[q];
    if (u < 0 || u >= n_users) {  // no training row: the host adds nothing
        if (lane == 0) {
            out_ub[q] = 0.0f;
            out_add[q] = 0;
        }
        return;
    }
    const int64_t s = (int64_t)indptr[u];
    const int64_t n = (int64_t)indptr[u + 1] - s;
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
    if (lane == 0) {
        double ub = (double)total / ((double)cnt + damping);
        if (__builtin_isnan(ub)) ub = 0.0;
        out_ub[q] = (float)ub;
        out_add[q] = 1;
    }
}

__global__ __launch_bounds__(256) void predict_merge_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items,
    int64_t n_entries, int64_t n_items, float *__restrict__ scores,
    const float *__restrict__ item_means, int fallback, float global_bias,
    const float *__restrict__ item_biases, const float *__restrict__ user_bias,
    const uint8_t *__restrict__ user_add, uint8_t *__restrict__ out_fb)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    const int32_t t = tgt_items[e];
    const bool known = t >= 0 && t < n_items;
    float s = scores[e];
    if (item_means && known) s = s + item_means[t];  // item.py:282
    uint8_t fb = 0;
    if (fallback && __builtin_isnan(s)) {
        s = global_bias;  // np.full(n, mu, float32)
        if (item_biases && known) s = s + item_biases[t];
        if (user_add) {
            // the entry's query: the last q with tgt_ptr[q] <= e (empty lists hold no entries)
            int64_t lo = 0, hi = n_queries - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (tgt_ptr[mid] <= e) lo = mid;
                else hi = mid - 1;
            }
            if (user_add[lo]) s = s + user_bias[lo];
        }
        fb = 1;
    }
    scores[e] = s;
    if (out_fb) out_fb[e] = fb;
}

}  // namespace
}  // namespace lk

extern "C" int lk_bias_user_offsets(const void *d_indptr, int indptr_is_64,
                                    const int32_t *d_indices, const float *d_values,
                                    int64_t n_users, int64_t n_items, int64_t n_queries,
                                    const int32_t *d_user_nums, double global_bias,
                                    const float *d_item_biases, double damping_user,
                                    float *d_out_ub, uint8_t *d_out_add, void *stream)
{
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_queries >= 0,
               "lk_bias_user_offsets: negative size");
    if (n_queries == 0) return LK_OK;
    LK_REQUIRE(n_queries <= (int64_t)INT32_MAX, "lk_bias_user_offsets: too many queries");
    LK_REQUIRE(d_indptr && d_indices && d_values && d_user_nums && d_out_ub && d_out_add,
               "lk_bias_user_offsets: null pointer");
    hipStream_t st = lk::as_stream(stream);
    const lk::UoffSrc src{d_indices, d_values, d_item_biases, n_items, global_bias};
    const dim3 grid((unsigned)n_queries), block(lk::WAVE);
    if (indptr_is_64)
        hipLaunchKernelGGL(lk::bias_user_offsets_kernel<int64_t>, grid, block, 0, st,
                           static_cast<const int64_t *>(d_indptr), src, n_users, n_queries,
                           d_user_nums, damping_user, d_out_ub, d_out_add);
    else
        hipLaunchKernelGGL(lk::bias_user_offsets_kernel<int32_t>, grid, block, 0, st,
                           static_cast<const int32_t *>(d_indptr), src, n_users, n_queries,
                           d_user_nums, damping_user, d_out_ub, d_out_add);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_predict_merge(int64_t n_queries, const int64_t *d_tgt_ptr,
                                const int32_t *d_tgt_items, int64_t n_entries, int64_t n_items,
                                float *d_scores, const float *d_item_means, int fallback,
                                double global_bias, const float *d_item_biases,
                                const float *d_user_bias, const uint8_t *d_user_add,
                                uint8_t *d_out_is_fallback, void *stream)
{
    LK_REQUIRE(n_queries >= 0 && n_entries >= 0 && n_items >= 0,
               "lk_predict_merge: negative size");
    if (n_entries == 0) return LK_OK;
    LK_REQUIRE(n_queries > 0 && d_tgt_ptr && d_tgt_items && d_scores,
               "lk_predict_merge: null pointer");
    LK_REQUIRE(!d_user_add || d_user_bias, "lk_predict_merge: user flags without user biases");
    hipStream_t st = lk::as_stream(stream);
    const int64_t nb = (n_entries + 255) / 256;
    LK_REQUIRE(nb <= (int64_t)INT32_MAX, "lk_predict_merge: too many entries");
    hipLaunchKernelGGL(lk::predict_merge_kernel, dim3((unsigned)nb), dim3(256), 0, st, n_queries,
                       d_tgt_ptr, d_tgt_items, n_entries, n_items, d_scores, d_item_means,
                       fallback ? 1 : 0, (float)global_bias, d_item_biases, d_user_bias,
                       d_user_add, d_out_is_fallback);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
