// diversity.hip -- exposure, diversity, popularity and reranking metrics on the device: the
// per-item exposure totals of the Gini metrics (lk_item_exposure), the per-list category column
// sums behind ILS / Entropy / RankBiasedEntropy (lk_list_category_stats), MeanPopRank's gathered
// sum (lk_list_gather_mean) and the pairwise statistics of rank-biased overlap and
// least-item-promoted (lk_list_pair_stats).  The metric VALUES are composed on the host
// (lkpy_amd/metrics.py, lkpy_amd/reranking_metrics.py); see include/lkamd.h for the contract.
//
// Every float64 sum whose order the contract fixes is added by ONE chain in that order; products
// and sums are separate roundings: the file is compiled with contraction off, and the arithmetic
// is written out here (an inlined helper from a header compiled with contraction on would bring
// its `contract` flag along and fuse again).  No floating-point atomics.
#include "common.h"
#include "radix_sort.h"

#pragma clang fp contract(off)  // w * v is rounded before it is added, as NumPy does it

namespace lk {
namespace {

constexpr int DV_MAX_CATS = 7168;   // category columns of lk_list_category_stats (56 KiB of LDS)
constexpr int DV_MAX_DEPTH = 1024;  // depth n of lk_list_pair_stats
constexpr int DV_SLOTS = 2048;      // hash slots of lk_list_pair_stats: 2 x DV_MAX_DEPTH

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// ---- lk_item_exposure -----------------------------------------------------------------------
// One wave per list: entry (list q, column c) -> key = its item when the entry counts (kept,
// inside the cutoff, a known item), else the sentinel n_items; value = its rank.  The pairs are
// written at q * len + c: list order, then rank order -- the order a stable sort keeps.
__global__ __launch_bounds__(256) void exposure_keys_kernel(
    const int32_t *__restrict__ lists, int64_t n_lists, int64_t ld, int64_t len, int32_t cutoff,
    int32_t n_items, unsigned *__restrict__ keys, unsigned *__restrict__ ranks)
{
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_lists) return;
    const int32_t *row = lists + q * ld;
    int kept_before = 0;
    for (int64_t base = 0; base < len; base += WAVE) {
        const int64_t col = base + lane;
        const int32_t item = col < len ? row[col] : -1;
        const bool kept = item >= 0;
        const unsigned long long km = __ballot(kept);
        const int rank = kept_before + __popcll(km & ((1ull << lane) - 1ull)) + 1;
        if (col < len) {
            const bool counts = kept && item < n_items && (cutoff == 0 || rank <= cutoff);
            keys[q * len + col] = counts ? (unsigned)item : (unsigned)n_items;
            ranks[q * len + col] = (unsigned)rank;
        }
        kept_before += __popcll(km);
    }
}

// first position of the ascending keys[0, n) that is >= key
__device__ __forceinline__ int64_t lower_bound_u32(const unsigned *__restrict__ keys, int64_t n,
                                                   unsigned key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One wave per item: its run of the sorted pairs is found by two binary searches; the lanes load
// 64 weights of the run at a time and every lane adds them, one after the other in run order, to
// the same running total that starts at totals[item] -- the loads are spread over the wave, the
// additions are the single chain `totals[item] += w` of the reference (GiniAccumulator.add).
__global__ __launch_bounds__(256) void exposure_sum_kernel(
    const unsigned *__restrict__ keys, const unsigned *__restrict__ ranks, int64_t n,
    int32_t n_items, const double *__restrict__ W, double *__restrict__ totals)
{
    const int lane = lane_id();
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const int64_t p0 = lower_bound_u32(keys, n, (unsigned)item);
    const int64_t p1 = lower_bound_u32(keys, n, (unsigned)item + 1u);
    if (p1 <= p0) return;
    double acc = totals[item];
    for (int64_t base = p0; base < p1; base += WAVE) {
        const int64_t p = base + lane;
        double w = 0.0;
        if (p < p1) w = W ? W[ranks[p] - 1u] : 1.0;
        const int cnt = p1 - base < WAVE ? (int)(p1 - base) : WAVE;
        for (int l = 0; l < cnt; ++l) acc += __shfl(w, l, WAVE);
    }
    if (lane == 0) totals[item] = acc;
}

struct ExposureWs {
    size_t keys_in, vals_in, keys_out, vals_out, keys_tmp, vals_tmp, temp, total;
};

ExposureWs exposure_ws(int64_t n)
{
    ExposureWs w;
    const size_t arr = align_up((size_t)(n > 0 ? n : 1) * sizeof(unsigned), 256);
    w.keys_in = 0;
    w.vals_in = arr;
    w.keys_out = 2 * arr;
    w.vals_out = 3 * arr;
    w.keys_tmp = 4 * arr;
    w.vals_tmp = 5 * arr;
    w.temp = 6 * arr;
    w.total = w.temp + radix_sort_temp_bytes(n);
    return w;
}

// ---- lk_list_category_stats -----------------------------------------------------------------
// One wave (= one workgroup) per list, the C column sums in LDS.  The kept items inside the
// cutoff are walked in rank order; the lanes spread over ONE item's matrix row (distinct columns:
// distinct cells), each doing a plain read / add / write, so every cell sees the additions of a
// sequential column sum, in rank order.
__global__ __launch_bounds__(64) void category_stats_kernel(
    const int32_t *__restrict__ lists, int64_t n_lists, int64_t ld, int64_t len, int32_t cutoff,
    int32_t n_items, const int64_t *__restrict__ cptr, const int32_t *__restrict__ ccols,
    const double *__restrict__ cvals, int32_t n_cats, const double *__restrict__ W,
    int32_t *__restrict__ out_known, double *__restrict__ out_d)
{
    extern __shared__ double s_col[];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int c = lane; c < n_cats; c += WAVE) s_col[c] = 0.0;
    wave_lds_sync();
    const int32_t *row = lists + q * ld;
    int kept_before = 0, known = 0;
    double self = 0.0;
    for (int64_t base = 0; base < len; base += WAVE) {
        const int64_t col = base + lane;
        const int32_t item = col < len ? row[col] : -1;
        const bool kept = item >= 0;
        const unsigned long long km = __ballot(kept);
        const int rank = kept_before + __popcll(km & ((1ull << lane) - 1ull)) + 1;
        unsigned long long m = __ballot(kept && item < n_items && (cutoff == 0 || rank <= cutoff));
        while (m) {  // wave-uniform: ascending lane = ascending rank
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const int32_t it = __shfl(item, l, WAVE);
            const int r = __shfl(rank, l, WAVE);
            const double w = W ? W[r - 1] : 1.0;
            const int64_t e1 = cptr[it + 1];
            for (int64_t e = cptr[it] + lane; e < e1; e += WAVE) {
                const double v = cvals[e];
                const int32_t c = ccols[e];
                if (c >= 0 && c < n_cats) s_col[c] += w * v;
                self += v * v;
            }
            ++known;
            wave_lds_sync();  // the next item may touch the same cells from other lanes
        }
        kept_before += __popcll(km);
    }
    double sq = 0.0, tot = 0.0;
    for (int c = lane; c < n_cats; c += WAVE) {
        const double s = s_col[c];
        sq += s * s;
        tot += s + 1e-6;
    }
    sq = wave_sum_f64(sq);
    tot = wave_sum_f64(tot);
    self = wave_sum_f64(self);
    double ent = 0.0;  // matrix_column_entropy: p = (s + 1e-6) / sum(s + 1e-6), -sum p log2 p
    for (int c = lane; c < n_cats; c += WAVE) {
        const double p = (s_col[c] + 1e-6) / tot;
        ent += p * log2(p);
    }
    ent = -wave_sum_f64(ent);
    if (lane == 0) {
        out_known[q] = known;
        out_d[q] = sq;
        out_d[n_lists + q] = self;
        out_d[2 * n_lists + q] = ent;
    }
}

// ---- lk_list_gather_mean --------------------------------------------------------------------
// One wave per list: table[item] over the kept entries inside the cutoff, added in rank order.
__global__ __launch_bounds__(256) void gather_mean_kernel(
    const int32_t *__restrict__ lists, int64_t n_lists, int64_t ld, int64_t len, int32_t cutoff,
    const double *__restrict__ table, int32_t n_items, double *__restrict__ out_sum,
    int32_t *__restrict__ out_len)
{
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_lists) return;
    const int32_t *row = lists + q * ld;
    int kept_before = 0, used = 0;
    double acc = 0.0;
    for (int64_t base = 0; base < len; base += WAVE) {
        const int64_t col = base + lane;
        const int32_t item = col < len ? row[col] : -1;
        const bool kept = item >= 0;
        const unsigned long long km = __ballot(kept);
        const int rank = kept_before + __popcll(km & ((1ull << lane) - 1ull)) + 1;
        const bool in = kept && (cutoff == 0 || rank <= cutoff);
        const double v = (in && item < n_items) ? table[item] : 0.0;  // unknown: 0, but counted
        const unsigned long long m = __ballot(in);
        used += __popcll(m);
        unsigned long long walk = m;
        while (walk) {
            const int l = __builtin_ctzll(walk);
            walk &= walk - 1ull;
            acc += __shfl(v, l, WAVE);
        }
        kept_before += __popcll(km);
    }
    if (lane == 0) {
        out_sum[q] = acc;
        out_len[q] = used;
    }
}

// ---- lk_list_pair_stats ---------------------------------------------------------------------
__device__ __forceinline__ unsigned pair_hash(int32_t x)
{
    return ((unsigned)x * 2654435761u) >> 21;  // 11 bits: DV_SLOTS
}

// One wave (= one workgroup) per pair.  b[:n] goes into an LDS hash table (item -> position in b;
// at most half full, so every probe sequence ends at an empty slot), then `a` is scanned ONCE: an
// item of a found in b[:n] raises the least-item-promoted maximum, and -- when it lies in a[:n]
// too -- counts in the histogram over max(rank_a, rank_b), whose prefix sum is overlap_d.
__global__ __launch_bounds__(64) void pair_stats_kernel(
    int64_t n_pairs, const int32_t *__restrict__ a_rows, const int64_t *__restrict__ a_ptr,
    const int32_t *__restrict__ a_items, const int64_t *__restrict__ b_ptr,
    const int32_t *__restrict__ b_items, int32_t n, const double *__restrict__ W,
    double *__restrict__ out_rbo, int32_t *__restrict__ out_lip, int32_t *__restrict__ out_flag)
{
    __shared__ int32_t s_key[DV_SLOTS];
    __shared__ int32_t s_pos[DV_SLOTS];
    __shared__ int32_t s_hist[DV_MAX_DEPTH + 1];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int i = lane; i < DV_SLOTS; i += WAVE) s_key[i] = -1;
    for (int i = lane; i <= n; i += WAVE) s_hist[i] = 0;
    __syncthreads();
    const int64_t ar = a_rows ? (int64_t)a_rows[q] : q;
    int64_t a0 = 0, a1 = 0;
    if (ar >= 0) {
        a0 = a_ptr[ar];
        a1 = a_ptr[ar + 1];
    }
    const int64_t b0 = b_ptr[q];
    const int64_t nb = b_ptr[q + 1] - b0 < n ? b_ptr[q + 1] - b0 : (int64_t)n;
    for (int64_t i = lane; i < nb; i += WAVE) {
        const int32_t x = b_items[b0 + i];
        if (x < 0) continue;
        unsigned h = pair_hash(x);
        for (;;) {
            const int32_t old = atomicCAS(&s_key[h], -1, x);
            if (old == -1) {
                s_pos[h] = (int32_t)i;
                break;
            }
            if (old == x) break;  // (a repeated item: its first position stays)
            h = (h + 1u) & (DV_SLOTS - 1);
        }
    }
    __syncthreads();
    int64_t far = -1;  // largest 0-based position in a of an item of b[:n]
    for (int64_t i = a0 + lane; i < a1; i += WAVE) {
        const int32_t x = a_items[i];
        if (x < 0) continue;
        unsigned h = pair_hash(x);
        int32_t k;
        while ((k = s_key[h]) != -1 && k != x) h = (h + 1u) & (DV_SLOTS - 1);
        if (k == x) {
            const int64_t pa = i - a0;
            if (pa > far) far = pa;
            if (pa < n) {
                const int32_t pb = s_pos[h];
                atomicAdd(&s_hist[(pa > pb ? (int32_t)pa : pb) + 1], 1);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t o = __shfl_xor(far, off, WAVE);
        far = o > far ? o : far;
    }
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;  // _rbo.py:45-55: sum += (overlap / d) * w, d = 1 .. n
        int overlap = 0;
        for (int d = 1; d <= n; ++d) {
            overlap += s_hist[d];
            sum += ((double)overlap / (double)d) * W[d - 1];
        }
        out_rbo[q] = sum;
        out_lip[q] = (int32_t)((far > n ? far : (int64_t)n) - n);  // _lip.py:41-48
        out_flag[q] = a1 == a0 ? 1 : 0;
    }
}

}  // namespace
}  // namespace lk

extern "C" int32_t lk_list_category_max(void) { return lk::DV_MAX_CATS; }

extern "C" size_t lk_item_exposure_workspace_bytes(int64_t n_lists, int64_t len)
{
    if (n_lists <= 0 || len <= 0) return 0;
    return lk::exposure_ws(n_lists * len).total;
}

extern "C" int lk_item_exposure(const int32_t *d_lists, int64_t n_lists, int64_t ld, int64_t len,
                                int32_t cutoff, const double *d_weights, int64_t w_ld,
                                int32_t n_items, double *d_totals, void *d_ws, void *stream)
{
    LK_REQUIRE(n_lists >= 0 && ld >= 0 && len >= 0 && len <= ld,
               "lk_item_exposure: bad list shape");
    LK_REQUIRE(cutoff >= 0 && n_items >= 0, "lk_item_exposure: negative cutoff or item count");
    LK_REQUIRE(!d_weights || w_ld >= (cutoff > 0 && cutoff < len ? (int64_t)cutoff : len),
               "lk_item_exposure: weight table shorter than the lists");
    if (n_lists == 0 || len == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_lists && d_totals && d_ws, "lk_item_exposure: null pointer");
    LK_REQUIRE(n_lists <= (int64_t)INT32_MAX && n_lists * len < ((int64_t)1 << 40),
               "lk_item_exposure: too many entries");
    const int64_t n = n_lists * len;
    const lk::ExposureWs w = lk::exposure_ws(n);
    char *ws = static_cast<char *>(d_ws);
    auto at = [&](size_t off) { return reinterpret_cast<unsigned *>(ws + off); };
    hipStream_t st = lk::as_stream(stream);
    hipLaunchKernelGGL(lk::exposure_keys_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0,
                       st, d_lists, n_lists, ld, len, cutoff, n_items, at(w.keys_in),
                       at(w.vals_in));
    LK_HIP_CHECK(hipGetLastError());
    int bits = 1;  // the keys are 0 .. n_items (the sentinel)
    while (bits < 32 && ((int64_t)1 << bits) <= (int64_t)n_items) ++bits;
    const int rc = lk::radix_sort_pairs<unsigned, unsigned>(
        at(w.keys_in), at(w.vals_in), at(w.keys_out), at(w.vals_out), at(w.keys_tmp),
        at(w.vals_tmp), n, 0, bits, ws + w.temp, st);
    if (rc != LK_OK) return rc;
    hipLaunchKernelGGL(lk::exposure_sum_kernel, dim3((unsigned)(((int64_t)n_items + 3) / 4)),
                       dim3(256), 0, st, at(w.keys_out), at(w.vals_out), n, n_items, d_weights,
                       d_totals);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_list_category_stats(const int32_t *d_lists, int64_t n_lists, int64_t ld,
                                      int64_t len, int32_t cutoff, int32_t n_items,
                                      const int64_t *d_cat_ptr, const int32_t *d_cat_cols,
                                      const double *d_cat_vals, int32_t n_cats,
                                      const double *d_weights, int64_t w_ld, int32_t *d_out_known,
                                      double *d_out_stats, void *stream)
{
    LK_REQUIRE(n_lists >= 0 && ld >= 0 && len >= 0 && len <= ld,
               "lk_list_category_stats: bad list shape");
    LK_REQUIRE(cutoff >= 0 && n_items >= 0, "lk_list_category_stats: negative cutoff or item count");
    LK_REQUIRE(n_cats >= 1 && n_cats <= lk::DV_MAX_CATS,
               "lk_list_category_stats: 1..%d category columns", lk::DV_MAX_CATS);
    LK_REQUIRE(!d_weights || w_ld >= (cutoff > 0 && cutoff < len ? (int64_t)cutoff : len),
               "lk_list_category_stats: weight table shorter than the lists");
    if (n_lists == 0) return LK_OK;
    LK_REQUIRE((len == 0 || d_lists) && d_cat_ptr && d_out_known && d_out_stats,
               "lk_list_category_stats: null pointer");
    LK_REQUIRE(n_lists <= (int64_t)INT32_MAX, "lk_list_category_stats: too many lists");
    hipLaunchKernelGGL(lk::category_stats_kernel, dim3((unsigned)n_lists), dim3(64),
                       (size_t)n_cats * sizeof(double), lk::as_stream(stream), d_lists, n_lists, ld,
                       len, cutoff, n_items, d_cat_ptr, d_cat_cols, d_cat_vals, n_cats, d_weights,
                       d_out_known, d_out_stats);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_list_gather_mean(const int32_t *d_lists, int64_t n_lists, int64_t ld,
                                   int64_t len, int32_t cutoff, const double *d_table,
                                   int32_t n_items, double *d_out_sum, int32_t *d_out_len,
                                   void *stream)
{
    LK_REQUIRE(n_lists >= 0 && ld >= 0 && len >= 0 && len <= ld,
               "lk_list_gather_mean: bad list shape");
    LK_REQUIRE(cutoff >= 0 && n_items >= 0, "lk_list_gather_mean: negative cutoff or item count");
    if (n_lists == 0) return LK_OK;
    LK_REQUIRE((len == 0 || d_lists) && (n_items == 0 || d_table) && d_out_sum && d_out_len,
               "lk_list_gather_mean: null pointer");
    LK_REQUIRE(n_lists <= (int64_t)INT32_MAX, "lk_list_gather_mean: too many lists");
    hipLaunchKernelGGL(lk::gather_mean_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0,
                       lk::as_stream(stream), d_lists, n_lists, ld, len, cutoff, d_table, n_items,
                       d_out_sum, d_out_len);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_list_pair_stats(int64_t n_pairs, const int32_t *d_a_rows,
                                  const int64_t *d_a_ptr, const int32_t *d_a_items,
                                  const int64_t *d_b_ptr, const int32_t *d_b_items, int32_t n,
                                  const double *d_weights, double *d_out_rbo, int32_t *d_out_lip,
                                  int32_t *d_out_flag, void *stream)
{
    LK_REQUIRE(n_pairs >= 0, "lk_list_pair_stats: negative size");
    LK_REQUIRE(n >= 1 && n <= lk::DV_MAX_DEPTH, "lk_list_pair_stats: depth 1..%d",
               lk::DV_MAX_DEPTH);
    if (n_pairs == 0) return LK_OK;
    LK_REQUIRE(d_a_ptr && d_b_ptr && d_weights && d_out_rbo && d_out_lip && d_out_flag,
               "lk_list_pair_stats: null pointer");
    LK_REQUIRE(n_pairs <= (int64_t)INT32_MAX, "lk_list_pair_stats: too many pairs");
    hipLaunchKernelGGL(lk::pair_stats_kernel, dim3((unsigned)n_pairs), dim3(64), 0,
                       lk::as_stream(stream), n_pairs, d_a_rows, d_a_ptr, d_a_items, d_b_ptr,
                       d_b_items, n, d_weights, d_out_rbo, d_out_lip, d_out_flag);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
