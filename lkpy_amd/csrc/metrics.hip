// metrics.hip -- run evaluation on the device: the sufficient statistics of the ranking metrics
// (lk_rank_stats), graded NDCG's ideal gain (lk_ideal_gain) and the prediction errors
// (lk_predict_errors).  The metric VALUES are composed on the host from these statistics with the
// reference's own expressions (lkpy_amd/metrics.py); see include/lkamd.h for the contract.
//
// Every float64 sum is added in rank (list) order by a wave-uniform loop over the bits of a
// __ballot mask: the result depends on the list and its truth row alone -- not on the batch, the
// launch shape or the run.  No floating-point atomics.
#include "common.h"

namespace lk {
namespace {

constexpr int MT_MAX_CUT = 8;     // cutoffs of one lk_rank_stats launch / combos of lk_ideal_gain
constexpr int MT_MAX_TAB = 4;     // rank-weight tables of one launch
constexpr int MT_LDS_ROW = 4096;  // longest truth row lk_ideal_gain sorts in LDS

struct MtInts {
    int32_t v[MT_MAX_CUT];
};

// v[i] without a dynamically indexed copy of the kernel argument (that would live in scratch)
__device__ __forceinline__ int32_t pick(const MtInts &a, int i)
{
    int32_t r = a.v[0];
#pragma unroll
    for (int k = 1; k < MT_MAX_CUT; ++k) r = (i == k) ? a.v[k] : r;
    return r;
}

// position of `item` in the ascending, duplicate-free row items[lo, hi), or -1
__device__ __forceinline__ int64_t find_item(const int32_t *__restrict__ items, int64_t lo,
                                             int64_t hi, int32_t item)
{
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (items[mid] < item) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && items[lo] == item) ? lo : -1;
}

// One wave per list.  Lane j < n_cut keeps the integer statistics of cutoff j; lane
// j < n_cut * (1 + 2 n_tab) keeps ONE float64 sum: field j = (cutoff j / per, kind j % per) with
// kind 0 = ap_sum, 1 + 2t = w_hits of table t, 2 + 2t = g_hits of table t.  The hits of a trip
// are walked in rank order by every lane together; a lane adds the hit's term to its own sum
// when the hit's rank is inside its cutoff (the hits inside a cutoff are a prefix of the hits,
// so the running hit count is the count inside the cutoff as well).
__global__ __launch_bounds__(256) void rank_stats_kernel(
    const int32_t *__restrict__ lists, int64_t n_lists, int64_t ld, int64_t len,
    const int64_t *__restrict__ tptr, const int32_t *__restrict__ titems,
    const float *__restrict__ tgains, MtInts cuts, int n_cut, const double *__restrict__ W,
    int n_tab, int64_t w_ld, int32_t *__restrict__ out_i, double *__restrict__ out_d)
{
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_lists) return;  // (the whole wave; the kernel has no workgroup barrier)
    const int per = 1 + 2 * n_tab;
    const bool f_on = lane < n_cut * per;
    const int fk = lane % per;
    const int32_t f_n = f_on ? pick(cuts, lane / per) : 0;
    const double *f_w = W + (int64_t)(fk > 0 ? (fk - 1) >> 1 : 0) * w_ld;
    const bool f_graded = fk > 0 && ((fk - 1) & 1);
    const bool i_on = lane < n_cut;
    const int32_t i_n = i_on ? pick(cuts, lane) : 0;
    const int64_t t0 = tptr[q], t1 = tptr[q + 1];
    const int32_t *row = lists + q * ld;

    double acc = 0.0;
    int n_hits = 0, first = 0, kept_before = 0, cum = 0;
    for (int64_t base = 0; base < len; base += WAVE) {
        const int64_t col = base + lane;
        const int32_t item = col < len ? row[col] : -1;
        const bool kept = item >= 0;  // padding / unknown items are dropped before ranking
        const unsigned long long km = __ballot(kept);
        const int rank = kept_before + __popcll(km & ((1ull << lane) - 1ull)) + 1;
        const int64_t pos = kept ? find_item(titems, t0, t1, item) : -1;
        const bool hit = pos >= 0;
        float gain = 1.0f;
        if (hit && tgains) gain = tgains[pos];
        const int g_ok = __builtin_isnan(gain) ? 0 : 1;  // NaN gain: not in the graded test data
        const double gv = g_ok ? (double)fmaxf(gain, 0.0f) : 0.0;
        unsigned long long hm = __ballot(hit);
        while (hm) {  // wave-uniform: ascending lane = ascending rank
            const int l = __builtin_ctzll(hm);
            hm &= hm - 1ull;
            const int r = __shfl(rank, l, WAVE);
            const double g = __shfl(gv, l, WAVE);
            const int ok = __shfl(g_ok, l, WAVE);
            ++cum;
            if (f_on && (f_n == 0 || r <= f_n)) {
                if (fk == 0) acc += (double)cum / (double)r;  // _map.py:37-41
                else {
                    const double w = f_w[r - 1];
                    if (!f_graded) acc += w;                  // _binary_dcg, rank_biased_precision
                    else if (tgains && ok) acc += g * w;      // _graded_dcg
                }
            }
            if (i_on && (i_n == 0 || r <= i_n)) {
                ++n_hits;
                if (!first) first = r;
            }
        }
        kept_before += __popcll(km);
    }
    if (lane == 0) {
        out_i[q] = kept_before;
        out_i[n_lists + q] = (int32_t)(t1 - t0);
    }
    if (i_on) {
        out_i[(int64_t)(2 + 2 * lane) * n_lists + q] = n_hits;
        out_i[(int64_t)(3 + 2 * lane) * n_lists + q] = first;
    }
    if (f_on) out_d[(int64_t)lane * n_lists + q] = acc;
}

// One workgroup per truth row: order-preserving keys of the clipped gains (NaN -> key 0, below
// every real key) sorted descending by a bitonic network -- in LDS for rows up to MT_LDS_ROW, in
// the row's slab of the workspace beyond -- then thread c adds combo c's products in that order.
template <bool LONG>
__global__ __launch_bounds__(256) void ideal_gain_kernel(
    const int64_t *__restrict__ tptr, const float *__restrict__ gains, int64_t n_rows,
    const int32_t *__restrict__ long_rows, unsigned *ws, int64_t slab, MtInts cuts,
    MtInts tabs, int n_combo, const double *__restrict__ W, int64_t w_ld,
    double *__restrict__ out_d, int32_t *__restrict__ out_cnt)
{
    __shared__ unsigned s_keys[LONG ? 1 : MT_LDS_ROW];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int64_t r = LONG ? (int64_t)long_rows[blockIdx.x] : (int64_t)blockIdx.x;
    if (r < 0 || r >= n_rows) return;
    const int64_t t0 = tptr[r];
    const int64_t len = tptr[r + 1] - t0;
    if (LONG ? (len > slab) : (len > MT_LDS_ROW)) return;  // (uniform; the other launch's row)
    unsigned *buf = LONG ? ws + (int64_t)blockIdx.x * slab : s_keys;
    int64_t P = 1;
    while (P < len) P <<= 1;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int64_t i = tid; i < P; i += 256) {
        unsigned key = 0u;
        if (i < len) {
            const float g = gains[t0 + i];
            if (!__builtin_isnan(g)) {  // dropna, then clip(lower=0): _dcg.py:122-127
                key = f2key(fmaxf(g, 0.0f));
                ++mine;
            }
        }
        buf[i] = key;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __threadfence_block();
    __syncthreads();
    for (int64_t k = 2; k <= P; k <<= 1)
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = tid; i < P; i += 256) {
                const int64_t x = i ^ j;
                if (x > i) {
                    const unsigned a = buf[i], b = buf[x];
                    const bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) {
                        buf[i] = b;
                        buf[x] = a;
                    }
                }
            }
            // LONG: the exchange goes through global memory between the waves of ONE workgroup;
            // the workgroup-scope fence makes this stage's stores visible to them after the barrier
            __threadfence_block();
            __syncthreads();
        }
    const int cnt = s_cnt;
    if (tid < n_combo) {
        const int32_t n = pick(cuts, tid);
        int64_t terms = cnt;
        if (n > 0 && n < terms) terms = n;  // nlargest(n) / sort_values(ascending=False)
        if (terms > w_ld) terms = w_ld;
        const double *w = W + (int64_t)pick(tabs, tid) * w_ld;
        double acc = 0.0;
        for (int64_t i = 0; i < terms; ++i) acc += (double)key2f(buf[i]) * w[i];
        out_d[(int64_t)tid * n_rows + r] = acc;
    }
    if (tid == 0) out_cnt[r] = cnt;
}

// One wave per prediction list (its items distinct: a repeated item would be matched to its
// truth entry once per occurrence and n_missing_score would come out too small): every entry's
// rating is looked up in the truth row (or taken from the list's own rating array), e = score - rating and e*e / |e| are float32 operations as
// on two float32 series, and the float64 sums take them in list order.
__global__ __launch_bounds__(256) void predict_errors_kernel(
    int64_t n_lists, const int64_t *__restrict__ pptr, const int32_t *__restrict__ pitems,
    const float *__restrict__ pscores, const float *__restrict__ pratings,
    const int64_t *__restrict__ tptr, const int32_t *__restrict__ titems,
    const float *__restrict__ tratings, double *__restrict__ out_d, int32_t *__restrict__ out_i)
{
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_lists) return;
    const int64_t p0 = pptr[q], p1 = pptr[q + 1];
    int64_t t0 = 0, t1 = 0;
    if (tptr) {
        t0 = tptr[q];
        t1 = tptr[q + 1];
    }
    const float nanf_ = __builtin_nanf("");
    double sse = 0.0, sae = 0.0;
    int n = 0, matched = 0, miss_score = 0, miss_truth = 0;
    for (int64_t base = p0; base < p1; base += WAVE) {
        const int64_t i = base + lane;
        const bool act = i < p1;
        const float s = act ? pscores[i] : nanf_;
        float r = nanf_;
        if (act) {
            if (tptr) {
                const int32_t item = pitems[i];
                const int64_t pos = item >= 0 ? find_item(titems, t0, t1, item) : -1;
                if (pos >= 0) r = tratings[pos];
            } else {
                r = pratings[i];
            }
        }
        const bool s_ok = act && !__builtin_isnan(s);
        const bool r_ok = act && !__builtin_isnan(r);
        const bool both = s_ok && r_ok;
        const float e = s - r;
        const float e2 = e * e;
        const float ea = fabsf(e);
        const bool use = both && !__builtin_isnan(e);  // (inf - inf: skipped like any NaN)
        n += __popcll(__ballot(use && __builtin_isfinite(e)));
        matched += __popcll(__ballot(both));
        miss_truth += __popcll(__ballot(s_ok && !r_ok));
        miss_score += __popcll(__ballot(r_ok && !s_ok));
        unsigned long long m = __ballot(use);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            sse += (double)__shfl(e2, l, WAVE);
            sae += (double)__shfl(ea, l, WAVE);
        }
    }
    if (tptr) {  // rated in the truth, absent from the list or scored NaN
        int c = 0;
        for (int64_t i = t0 + lane; i < t1; i += WAVE) c += __builtin_isnan(tratings[i]) ? 0 : 1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, WAVE);
        miss_score = c - matched;
    }
    if (lane == 0) {
        out_d[q] = sse;
        out_d[n_lists + q] = sae;
        out_i[q] = n;
        out_i[n_lists + q] = miss_score;
        out_i[2 * n_lists + q] = miss_truth;
    }
}

int64_t pow2_ceil(int64_t x)
{
    int64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace
}  // namespace lk

extern "C" int lk_rank_stats(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                             const int64_t *d_truth_ptr, const int32_t *d_truth_items,
                             const float *d_truth_gains, const int32_t *cutoffs,
                             int32_t n_cutoffs, const double *d_weights, int32_t n_tables,
                             int64_t w_ld, int32_t *d_out_counts, double *d_out_sums,
                             void *stream)
{
    LK_REQUIRE(n_lists >= 0 && ld >= 0 && len >= 0 && len <= ld, "lk_rank_stats: bad list shape");
    LK_REQUIRE(n_cutoffs >= 1 && n_cutoffs <= lk::MT_MAX_CUT && cutoffs,
               "lk_rank_stats: 1..%d cutoffs", lk::MT_MAX_CUT);
    LK_REQUIRE(n_tables >= 0 && n_tables <= lk::MT_MAX_TAB, "lk_rank_stats: 0..%d weight tables",
               lk::MT_MAX_TAB);
    LK_REQUIRE(n_cutoffs * (1 + 2 * n_tables) <= lk::WAVE,
               "lk_rank_stats: cutoffs x (1 + 2 tables) must fit the 64 lanes of a wave");
    LK_REQUIRE(n_tables == 0 || (d_weights && w_ld >= len),
               "lk_rank_stats: weight tables shorter than the lists");
    if (n_lists == 0) return LK_OK;
    LK_REQUIRE((len == 0 || d_lists) && d_truth_ptr && d_out_counts && d_out_sums,
               "lk_rank_stats: null pointer");
    LK_REQUIRE(n_lists <= (int64_t)INT32_MAX, "lk_rank_stats: too many lists");
    lk::MtInts cuts = {};
    for (int i = 0; i < n_cutoffs; ++i) {
        LK_REQUIRE(cutoffs[i] >= 0, "lk_rank_stats: negative cutoff");
        cuts.v[i] = cutoffs[i];
    }
    hipLaunchKernelGGL(lk::rank_stats_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0,
                       lk::as_stream(stream), d_lists, n_lists, ld, len, d_truth_ptr,
                       d_truth_items, d_truth_gains, cuts, (int)n_cutoffs, d_weights,
                       (int)n_tables, w_ld, d_out_counts, d_out_sums);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" size_t lk_ideal_gain_workspace_bytes(int64_t n_long_rows, int64_t longest_row)
{
    if (n_long_rows <= 0 || longest_row <= lk::MT_LDS_ROW) return 0;
    return (size_t)n_long_rows * (size_t)lk::pow2_ceil(longest_row) * sizeof(unsigned);
}

extern "C" int lk_ideal_gain(const int64_t *d_truth_ptr, const float *d_gains, int64_t n_rows,
                             const int32_t *d_long_rows, int64_t n_long_rows, int64_t longest_row,
                             void *d_ws, const int32_t *cutoffs, const int32_t *tables,
                             int32_t n_combos, const double *d_weights, int32_t n_tables,
                             int64_t w_ld, double *d_out_ideal, int32_t *d_out_count,
                             void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n_long_rows >= 0 && longest_row >= 0, "lk_ideal_gain: negative size");
    LK_REQUIRE(n_combos >= 1 && n_combos <= lk::MT_MAX_CUT && cutoffs && tables,
               "lk_ideal_gain: 1..%d (cutoff, table) combinations", lk::MT_MAX_CUT);
    LK_REQUIRE(n_tables >= 1 && d_weights && w_ld >= 0, "lk_ideal_gain: no weight table");
    lk::MtInts cuts = {}, tabs = {};
    for (int i = 0; i < n_combos; ++i) {
        LK_REQUIRE(cutoffs[i] >= 0 && tables[i] >= 0 && tables[i] < n_tables,
                   "lk_ideal_gain: bad combination %d", i);
        cuts.v[i] = cutoffs[i];
        tabs.v[i] = tables[i];
    }
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_truth_ptr && d_gains && d_out_ideal && d_out_count, "lk_ideal_gain: null pointer");
    LK_REQUIRE(n_rows <= (int64_t)INT32_MAX && n_long_rows <= (int64_t)INT32_MAX,
               "lk_ideal_gain: too many rows");
    LK_REQUIRE(n_long_rows == 0 || (d_long_rows && d_ws), "lk_ideal_gain: long rows without workspace");
    hipStream_t st = lk::as_stream(stream);
    hipLaunchKernelGGL(lk::ideal_gain_kernel<false>, dim3((unsigned)n_rows), dim3(256), 0, st,
                       d_truth_ptr, d_gains, n_rows, d_long_rows, (unsigned *)nullptr, (int64_t)0,
                       cuts, tabs, (int)n_combos, d_weights, w_ld, d_out_ideal, d_out_count);
    LK_HIP_CHECK(hipGetLastError());
    if (n_long_rows > 0) {
        hipLaunchKernelGGL(lk::ideal_gain_kernel<true>, dim3((unsigned)n_long_rows), dim3(256), 0,
                           st, d_truth_ptr, d_gains, n_rows, d_long_rows,
                           static_cast<unsigned *>(d_ws), lk::pow2_ceil(longest_row), cuts, tabs,
                           (int)n_combos, d_weights, w_ld, d_out_ideal, d_out_count);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

extern "C" int lk_predict_errors(int64_t n_lists, const int64_t *d_pred_ptr,
                                 const int32_t *d_pred_items, const float *d_pred_scores,
                                 const float *d_pred_ratings, const int64_t *d_truth_ptr,
                                 const int32_t *d_truth_items, const float *d_truth_ratings,
                                 double *d_out_sums, int32_t *d_out_counts, void *stream)
{
    LK_REQUIRE(n_lists >= 0, "lk_predict_errors: negative size");
    if (n_lists == 0) return LK_OK;
    LK_REQUIRE(d_pred_ptr && d_out_sums && d_out_counts, "lk_predict_errors: null pointer");
    LK_REQUIRE(d_truth_ptr ? (d_pred_items != nullptr) : (d_pred_ratings != nullptr),
               "lk_predict_errors: neither a truth matrix nor the lists' own ratings");
    LK_REQUIRE(n_lists <= (int64_t)INT32_MAX, "lk_predict_errors: too many lists");
    hipLaunchKernelGGL(lk::predict_errors_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256),
                       0, lk::as_stream(stream), n_lists, d_pred_ptr, d_pred_items, d_pred_scores,
                       d_pred_ratings, d_truth_ptr, d_truth_items, d_truth_ratings, d_out_sums,
                       d_out_counts);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
