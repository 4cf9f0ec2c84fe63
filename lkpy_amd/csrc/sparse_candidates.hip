// sparse_candidates.hip -- per-query candidate lists for the scorers whose model is a sparse
// item-item matrix in HBM (SLIM: the transposed weights; association rules: the scores): the
// score of "THESE items for this query" without the dense [queries x items] panel that
// lk_slim_score_batch / lk_assoc_score_batch form.  The ragged target layout is that of
// candidates.hip: query q owns the positions [tgt_ptr[q], tgt_ptr[q + 1]) of one flat array.
//
//   rule     the score of target column c for query q: walk q's history in the order stored, skip
//            the items outside [0, n_items), count every other one in m (repeats included), and
//            where the item's model row holds column c fold that value into an accumulator that
//            starts at 0.f:
//              SUM   acc = acc + v        a history without entries gives NaN, else acc
//              MEAN  acc = acc + v        m == 0 gives NaN, else float(double(acc) / double(m))
//              MAX   acc = fmaxf(acc, v)  m == 0 gives NaN, else acc (absent cells count as 0)
//            A target outside [0, n_items) gives NaN.  The chain is one plain float32 addition
//            per history item in history order -- no partial sums, nothing fused -- which is the
//            cell `row[c] += v` of slim_score_kernel and the LDS cell of assoc_score_kernel, so a
//            result has the bits of that panel's entry.
//   kernel   a thread per target position, so a wave owns 64 consecutive positions whichever
//            queries they belong to; the thread finds its query by a binary search of the offsets
//            (query_of, as in candidates.hip), walks that query's history and looks its column up
//            in each model row by a binary search (columns ascend without repeats inside a row).
//            The lanes of one query read the same history entries and row bounds in the same
//            instruction (one request), probe the same rows, and their searches share the top
//            levels' lines.  Only the fold is ordered; the searches are not: GROUP history items
//            are looked up at a time, their probes issued together level by level (one memory
//            latency per level for the whole group), and the values found are folded in history
//            order afterwards.  No LDS, no barrier, no atomics; a result depends on its own
//            query's history and its own target alone.
//   bounds   every offset is clamped to its array's length, every row number and item number is
//            range-checked before it becomes an address; whatever the operands hold, no load
//            leaves hist_items[0, hist_nnz), the n_items + 1 model offsets or the model's
//            [0, model_nnz) entries.
#include "ragged.h"

namespace lk {
namespace sparsecand {

using ragged::clampi;
using ragged::query_of;

constexpr int THREADS = 256;
constexpr int GROUP = 8;  // history items whose searches are in flight together

template <int REDUCE>
__global__ __launch_bounds__(THREADS) void sparse_score_candidates_kernel(
    const int64_t *__restrict__ hist_ptr, const int32_t *__restrict__ hist_items,
    int64_t n_hist_rows, int64_t hist_nnz, const int32_t *__restrict__ rows, int64_t n_queries,
    const int64_t *__restrict__ m_ptr, const int32_t *__restrict__ m_idx,
    const float *__restrict__ m_val, int64_t n_items, int64_t model_nnz,
    const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items, int64_t total,
    float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= total) return;  // (the kernel has no barrier)
    const float nan = __builtin_nanf("");
    const int32_t c = tgt_items[t];
    if (c < 0 || c >= n_items) {
        out[t] = nan;
        return;
    }
    const int64_t q = query_of(tgt_ptr, n_queries, t);
    const int64_t r = rows ? (int64_t)rows[q] : q;
    int64_t hb = 0, he = 0;
    if (r >= 0 && r < n_hist_rows) {
        hb = clampi(hist_ptr[r], 0, hist_nnz);
        he = clampi(hist_ptr[r + 1], hb, hist_nnz);
    }

    float acc = 0.f;
    int64_t m = 0;  // known history items, repeats counted
    for (int64_t h0 = hb; h0 < he; h0 += GROUP) {
        // each step below is GROUP independent loads, issued together and waited for once
        int32_t it[GROUP];
        int64_t base[GROUP], end[GROUP];  // the item's model row
        int32_t len[GROUP], lo[GROUP], hi[GROUP];  // its length; the search, relative to base
        int32_t at[GROUP];  // the column at hi once hi has moved (-1 before: it matches no target)
        bool known[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) it[g] = h0 + g < he ? hist_items[h0 + g] : -1;
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            known[g] = it[g] >= 0 && it[g] < n_items;
            base[g] = known[g] ? m_ptr[it[g]] : 0;
            end[g] = known[g] ? m_ptr[it[g] + 1] : 0;
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            base[g] = clampi(base[g], 0, model_nnz);
            end[g] = clampi(end[g], base[g], model_nnz);
            len[g] = (int32_t)(end[g] - base[g] < INT32_MAX ? end[g] - base[g] : INT32_MAX);
            lo[g] = 0;
            hi[g] = len[g];
            at[g] = -1;
        }
        // GROUP lower bounds in lockstep: lo = hi = the first entry whose column is >= c
        bool more = true;
        while (more) {
            int32_t col[GROUP];
#pragma unroll
            for (int g = 0; g < GROUP; ++g)
                col[g] = lo[g] < hi[g] ? m_idx[base[g] + lo[g] + ((hi[g] - lo[g]) >> 1)] : 0;
            more = false;
#pragma unroll
            for (int g = 0; g < GROUP; ++g) {
                if (lo[g] < hi[g]) {
                    const int32_t mid = lo[g] + ((hi[g] - lo[g]) >> 1);
                    if (col[g] < c) {
                        lo[g] = mid + 1;
                    } else {
                        hi[g] = mid;
                        at[g] = col[g];
                    }
                }
                more |= lo[g] < hi[g];
            }
        }
        float v[GROUP];
        bool found[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) found[g] = at[g] == c;
#pragma unroll
        for (int g = 0; g < GROUP; ++g) v[g] = found[g] ? m_val[base[g] + lo[g]] : 0.f;
        // the fold, in history order (an unknown item is dropped: slim.py:133-134,
        // association.py:141-142)
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            m += known[g] ? 1 : 0;
            if (found[g]) acc = REDUCE == LK_SPARSE_MAX ? fmaxf(acc, v[g]) : acc + v[g];
        }
    }
    float res;
    if (REDUCE == LK_SPARSE_SUM) res = hb == he ? nan : acc;
    else if (REDUCE == LK_SPARSE_MEAN) res = m == 0 ? nan : (float)((double)acc / (double)m);
    else res = m == 0 ? nan : acc;
    out[t] = res;
}

}  // namespace sparsecand
}  // namespace lk

extern "C" int lk_sparse_score_candidates(
    const int64_t *d_hist_ptr, const int32_t *d_hist_items, int64_t n_hist_rows, int64_t hist_nnz,
    const int32_t *d_rows, int64_t n_queries, const int64_t *d_m_indptr,
    const int32_t *d_m_indices, const float *d_m_values, int64_t n_items, int64_t model_nnz,
    const int64_t *d_tgt_ptr, const int32_t *d_tgt_items, int64_t total, int reduce, float *d_out,
    void *stream)
{
    using namespace lk::sparsecand;
    LK_REQUIRE(n_hist_rows >= 0 && hist_nnz >= 0 && n_queries >= 0 && n_items >= 0 &&
                   model_nnz >= 0 && total >= 0 && n_items < ((int64_t)1 << 31),
               "lk_sparse_score_candidates: bad shape");
    LK_REQUIRE(reduce == LK_SPARSE_SUM || reduce == LK_SPARSE_MEAN || reduce == LK_SPARSE_MAX,
               "lk_sparse_score_candidates: unknown reduction %d", reduce);
    if (total == 0) return LK_OK;
    LK_REQUIRE(n_queries >= 1, "lk_sparse_score_candidates: targets without a query");
    LK_REQUIRE(d_tgt_ptr && d_tgt_items && d_out, "lk_sparse_score_candidates: null pointer");
    LK_REQUIRE((d_hist_ptr || n_hist_rows == 0) && (d_hist_items || hist_nnz == 0),
               "lk_sparse_score_candidates: null history");
    LK_REQUIRE((d_m_indptr || n_items == 0) && ((d_m_indices && d_m_values) || model_nnz == 0),
               "lk_sparse_score_candidates: null model");
    LK_REQUIRE(d_rows || n_hist_rows >= n_queries,
               "lk_sparse_score_candidates: without row numbers the history needs a row per query");
    const int64_t blocks = (total + THREADS - 1) / THREADS;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_sparse_score_candidates: too many targets");
    const dim3 grid((unsigned)blocks), block(THREADS);
    hipStream_t st = lk::as_stream(stream);
#define LK_SPARSE_LAUNCH(R)                                                                       \
    hipLaunchKernelGGL(sparse_score_candidates_kernel<R>, grid, block, 0, st, d_hist_ptr,         \
                       d_hist_items, n_hist_rows, hist_nnz, d_rows, n_queries, d_m_indptr,        \
                       d_m_indices, d_m_values, n_items, model_nnz, d_tgt_ptr, d_tgt_items,       \
                       total, d_out)
    if (reduce == LK_SPARSE_SUM) LK_SPARSE_LAUNCH(LK_SPARSE_SUM);
    else if (reduce == LK_SPARSE_MEAN) LK_SPARSE_LAUNCH(LK_SPARSE_MEAN);
    else LK_SPARSE_LAUNCH(LK_SPARSE_MAX);
#undef LK_SPARSE_LAUNCH
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
