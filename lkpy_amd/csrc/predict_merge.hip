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
// contiguous float64 array in its own pairwise order: bias_sum.h (shared with bmf_batch.hip).
#include "bias_sum.h"
#include "common.h"

// The host sums are plain adds and one divide; nothing may be fused.
#pragma clang fp contract(off)

namespace lk {
namespace {

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
    const double ub = row_user_bias(src, s, n, damping, tree);
    if (lane == 0) {
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
