// bias.hip -- the bias model on the device, gfx950: the fit of `BiasModel.learn`
// (src/lenskit/basic/bias.py:83-150) and the score of `BiasScorer` for whole batches.
//
//   bias_fit_short_kernel / bias_fit_long_kernel   one pass of the fit (lk_bias_fit_pass): for
//       every bin (an item's column of the transposed ratings, or a user's row) the two float64
//       chains `np.add.at` runs over the bin's entries in dataset order,
//           sum = 0.0 + (double)c[e0] + (double)c[e1] + ...      count = damping + 1.0 + 1.0 + ...
//       and b = (float)(sum / count) where count > 0, else 0.  c[e] = r[e] -f32 (float)mu, minus
//       (in float32) the other side's bias of the entry's column where the pass has one.  Neither
//       chain may be reassociated: `count` is not damping + n (the two differ from n = 223 on for
//       damping = 100 / 3), and the centred values lie on no common grid.  Bins are independent,
//       so there is no atomic anywhere: a bin of at most BIAS_SHORT entries is one lane's, a longer
//       one a wave's -- the wave loads BIAS_CHUNK entries at a time (coalesced, the next chunk in
//       flight while this one is added) and every lane runs the same chain over the chunk's values
//       lane by lane (v_readlane): what bounds the pass is the latency of the longest bin's chain.
//   bias_score_panel_kernel   score(q, i) = ((float)mu +f32 b_i) +f32 ub_q for a panel of queries,
//   bias_strike_kernel        NaN at each query's own training items (read by user number);
//   bias_score_ragged_kernel  the same cell at ragged targets; an unknown item's cell is
//                             (float)mu (+ ub_q), not NaN: `BiasModel.compute_for_items`.
#include "common.h"

// The host sums are plain adds and one divide; nothing may be fused.
#pragma clang fp contract(off)

namespace lk {
namespace {

// The two seams and the chain's step were chosen by measurement; the macros
// are there for tools/bias_variants.py to build the alternatives it times.
#ifndef LK_BIAS_SHORT
#define LK_BIAS_SHORT 64
#endif
#ifndef LK_BIAS_CHUNK
#define LK_BIAS_CHUNK 256
#endif
#ifndef LK_BIAS_LDS
#define LK_BIAS_LDS 0  // 1: the chunk's values laid in LDS as float64, the chain reads them there
#endif
constexpr int BIAS_SHORT = LK_BIAS_SHORT;  // bins up to this length: one lane each
constexpr int BIAS_CHUNK = LK_BIAS_CHUNK;  // longer bins: what a wave loads at a time
static_assert(BIAS_CHUNK % WAVE == 0 && BIAS_CHUNK >= WAVE, "a chunk is whole waves of entries");
constexpr int BIAS_PER_LANE = BIAS_CHUNK / WAVE;

struct FitSrc {
    const int32_t *indices;  // the entries' columns (read only with `sub`)
    const float *values;
    const float *sub;  // NULL: nothing but the global mean is subtracted
    int64_t n_sub;
    float mu;
};

// c[e]: float32 throughout, as the host's arrays are
template <bool SUB>
__device__ __forceinline__ float centred(const FitSrc &src, int64_t e)
{
    float c = src.values[e] - src.mu;
    if (SUB) {
        const int32_t j = src.indices[e];
        if (j >= 0 && j < src.n_sub) c = c - src.sub[j];
    }
    return c;
}

__device__ __forceinline__ float bias_of(double sum, double count)
{
    return count > 0.0 ? (float)(sum / count) : 0.0f;  // np.divide(..., where=counts > 0)
}

template <typename IT, bool SUB>
__global__ __launch_bounds__(256) void bias_fit_short_kernel(const IT *__restrict__ indptr,
                                                             FitSrc src, int64_t n_bins,
                                                             double damping,
                                                             float *__restrict__ out)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins) return;
    const int64_t s = (int64_t)indptr[b];
    const int64_t n = (int64_t)indptr[b + 1] - s;
    if (n > BIAS_SHORT) return;  // the long kernel's
    double sum = 0.0, count = damping;
    for (int64_t i = 0; i < n; ++i) {
        sum = sum + (double)centred<SUB>(src, s + i);
        count = count + 1.0;
    }
    out[b] = bias_of(sum, count);
}

template <bool SUB>
__device__ __forceinline__ void load_chunk(const FitSrc &src, int64_t base, int64_t end, int lane,
                                           float (&c)[BIAS_PER_LANE])
{
#pragma unroll
    for (int k = 0; k < BIAS_PER_LANE; ++k) {
        const int64_t e = base + k * WAVE + lane;
        c[k] = e < end ? centred<SUB>(src, e) : 0.0f;
    }
}

__device__ __forceinline__ double lane_value(float v, int lane)
{
    return (double)__builtin_bit_cast(
        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// One wave per bin; the waves of the short bins leave at once.
template <typename IT, bool SUB>
__global__ __launch_bounds__(256) void bias_fit_long_kernel(const IT *__restrict__ indptr,
                                                            FitSrc src, int64_t n_bins,
                                                            double damping,
                                                            float *__restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (b >= n_bins) return;
    const int64_t s = (int64_t)indptr[b];
    const int64_t end = (int64_t)indptr[b + 1];
    if (end - s <= BIAS_SHORT) return;
    double sum = 0.0, count = damping;
    float cur[BIAS_PER_LANE], nxt[BIAS_PER_LANE];
#if LK_BIAS_LDS
    __shared__ double stage[256 / WAVE][BIAS_CHUNK];
    double *mine = stage[threadIdx.x / WAVE];  // this wave's own: no workgroup barrier anywhere
#endif
    load_chunk<SUB>(src, s, end, lane, cur);
    for (int64_t base = s; base < end; base += BIAS_CHUNK) {
        const bool more = base + BIAS_CHUNK < end;
        if (more) load_chunk<SUB>(src, base + BIAS_CHUNK, end, lane, nxt);
#if LK_BIAS_LDS
        {
#pragma unroll
            for (int k = 0; k < BIAS_PER_LANE; ++k) mine[k * WAVE + lane] = (double)cur[k];
            wave_lds_sync();
            const int m = end - base < BIAS_CHUNK ? (int)(end - base) : BIAS_CHUNK;
            for (int t = 0; t < m; ++t) {
                sum = sum + mine[t];
                count = count + 1.0;
            }
            wave_lds_sync();  // (read before the next chunk overwrites it)
        }
#else
        if (end - base >= BIAS_CHUNK) {
#pragma unroll
            for (int k = 0; k < BIAS_PER_LANE; ++k) {
#pragma unroll
                for (int j = 0; j < WAVE; ++j) {
                    sum = sum + lane_value(cur[k], j);
                    count = count + 1.0;
                }
            }
        } else {
            const int m = (int)(end - base);
#pragma unroll
            for (int k = 0; k < BIAS_PER_LANE; ++k) {
                const int mk = m - k * WAVE < WAVE ? m - k * WAVE : WAVE;
                for (int j = 0; j < mk; ++j) {
                    sum = sum + lane_value(cur[k], j);
                    count = count + 1.0;
                }
            }
        }
#endif
        if (more) {
#pragma unroll
            for (int k = 0; k < BIAS_PER_LANE; ++k) cur[k] = nxt[k];
        }
    }
    if (lane == 0) out[b] = bias_of(sum, count);
}

template <typename IT, bool SUB>
int fit_pass(const IT *indptr, const FitSrc &src, int64_t n_bins, double damping, float *out,
             hipStream_t st)
{
    const int64_t nb_short = (n_bins + 255) / 256;
    const int64_t nb_long = (n_bins + 3) / 4;
    LK_REQUIRE(nb_long <= (int64_t)INT32_MAX, "lk_bias_fit_pass: too many bins");
    hipLaunchKernelGGL((bias_fit_short_kernel<IT, SUB>), dim3((unsigned)nb_short), dim3(256), 0,
                       st, indptr, src, n_bins, damping, out);
    LK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((bias_fit_long_kernel<IT, SUB>), dim3((unsigned)nb_long), dim3(256), 0, st,
                       indptr, src, n_bins, damping, out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ---- scoring --------------------------------------------------------------------------------
__device__ __forceinline__ float bias_cell(float mu, const float *item_biases, int64_t n_items,
                                           int32_t i, const float *ub, const uint8_t *add,
                                           int64_t q)
{
    float s = mu;  // np.full(n, mu, float32)
    if (item_biases && i >= 0 && i < n_items) s = s + item_biases[i];
    if (add && add[q]) s = s + ub[q];
    return s;
}

__global__ __launch_bounds__(256) void bias_score_panel_kernel(
    int64_t n_rows, int64_t n_items, float mu, const float *__restrict__ item_biases,
    const float *__restrict__ ub, const uint8_t *__restrict__ add, float *__restrict__ panel,
    int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    float base = mu;
    if (item_biases) base = base + item_biases[i];
    for (int64_t q = blockIdx.y; q < n_rows; q += gridDim.y) {
        float s = base;
        if (add && add[q]) s = s + ub[q];
        panel[q * ld + i] = s;
    }
}

template <typename IT>
__global__ __launch_bounds__(WAVE) void bias_strike_kernel(
    const IT *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n_users,
    const int32_t *__restrict__ user_nums, int64_t n_rows, int64_t n_items,
    float *__restrict__ panel, int64_t ld)
{
    const int64_t q = blockIdx.x;
    if (q >= n_rows) return;
    const int32_t u = user_nums[q];
    if (u < 0 || u >= n_users) return;
    const int64_t s = (int64_t)indptr[u], e = (int64_t)indptr[u + 1];
    for (int64_t p = s + threadIdx.x; p < e; p += WAVE) {
        const int32_t i = indices[p];
        if (i >= 0 && i < n_items) panel[q * ld + i] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void bias_score_ragged_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items,
    int64_t n_entries, int64_t n_items, float mu, const float *__restrict__ item_biases,
    const float *__restrict__ ub, const uint8_t *__restrict__ add, float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    int64_t lo = 0;
    if (add) {
        // the entry's query: the last q with tgt_ptr[q] <= e (empty lists hold no entries)
        int64_t hi = n_queries - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (tgt_ptr[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
    }
    out[e] = bias_cell(mu, item_biases, n_items, tgt_items[e], ub, add, lo);
}

}  // namespace
}  // namespace lk

extern "C" int32_t lk_bias_fit_short_max(void) { return lk::BIAS_SHORT; }
extern "C" int32_t lk_bias_fit_chunk(void) { return lk::BIAS_CHUNK; }

extern "C" int lk_bias_fit_pass(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                                const float *d_values, int64_t n_bins, double global_bias,
                                const float *d_sub, int64_t n_sub, double damping, float *d_out,
                                void *stream)
{
    LK_REQUIRE(n_bins >= 0 && n_sub >= 0, "lk_bias_fit_pass: negative size");
    if (n_bins == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_values && d_out, "lk_bias_fit_pass: null pointer");
    LK_REQUIRE(!d_sub || d_indices, "lk_bias_fit_pass: biases to subtract without the columns");
    hipStream_t st = lk::as_stream(stream);
    const lk::FitSrc src{d_indices, d_values, d_sub, n_sub, (float)global_bias};
    if (indptr_is_64) {
        const int64_t *p = static_cast<const int64_t *>(d_indptr);
        return d_sub ? lk::fit_pass<int64_t, true>(p, src, n_bins, damping, d_out, st)
                     : lk::fit_pass<int64_t, false>(p, src, n_bins, damping, d_out, st);
    }
    const int32_t *p = static_cast<const int32_t *>(d_indptr);
    return d_sub ? lk::fit_pass<int32_t, true>(p, src, n_bins, damping, d_out, st)
                 : lk::fit_pass<int32_t, false>(p, src, n_bins, damping, d_out, st);
}

extern "C" int lk_bias_score_panel(int64_t n_rows, int64_t n_items, double global_bias,
                                   const float *d_item_biases, const float *d_user_bias,
                                   const uint8_t *d_user_add, float *d_panel, int64_t ld,
                                   const void *d_hist_indptr, int indptr_is_64,
                                   const int32_t *d_hist_indices, int64_t n_users,
                                   const int32_t *d_user_nums, void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n_items >= 0 && n_users >= 0 && ld >= n_items,
               "lk_bias_score_panel: bad shape");
    if (n_rows == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(n_rows <= (int64_t)INT32_MAX, "lk_bias_score_panel: too many rows");
    LK_REQUIRE(d_panel, "lk_bias_score_panel: null pointer");
    LK_REQUIRE(!d_user_add || d_user_bias, "lk_bias_score_panel: user flags without user biases");
    LK_REQUIRE(!d_user_nums || (d_hist_indptr && d_hist_indices),
               "lk_bias_score_panel: histories to strike without their matrix");
    hipStream_t st = lk::as_stream(stream);
    const int64_t nbx = (n_items + 255) / 256;
    LK_REQUIRE(nbx <= (int64_t)INT32_MAX, "lk_bias_score_panel: too many items");
    const unsigned nby = (unsigned)(n_rows < 65535 ? n_rows : 65535);
    hipLaunchKernelGGL(lk::bias_score_panel_kernel, dim3((unsigned)nbx, nby), dim3(256), 0, st,
                       n_rows, n_items, (float)global_bias, d_item_biases, d_user_bias, d_user_add,
                       d_panel, ld);
    LK_HIP_CHECK(hipGetLastError());
    if (d_user_nums) {
        const dim3 grid((unsigned)n_rows), block(lk::WAVE);
        if (indptr_is_64)
            hipLaunchKernelGGL(lk::bias_strike_kernel<int64_t>, grid, block, 0, st,
                               static_cast<const int64_t *>(d_hist_indptr), d_hist_indices, n_users,
                               d_user_nums, n_rows, n_items, d_panel, ld);
        else
            hipLaunchKernelGGL(lk::bias_strike_kernel<int32_t>, grid, block, 0, st,
                               static_cast<const int32_t *>(d_hist_indptr), d_hist_indices, n_users,
                               d_user_nums, n_rows, n_items, d_panel, ld);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

extern "C" int lk_bias_score_ragged(int64_t n_queries, const int64_t *d_tgt_ptr,
                                    const int32_t *d_tgt_items, int64_t n_entries,
                                    int64_t n_items, double global_bias,
                                    const float *d_item_biases, const float *d_user_bias,
                                    const uint8_t *d_user_add, float *d_out, void *stream)
{
    LK_REQUIRE(n_queries >= 0 && n_entries >= 0 && n_items >= 0,
               "lk_bias_score_ragged: negative size");
    if (n_entries == 0) return LK_OK;
    LK_REQUIRE(n_queries > 0 && d_tgt_ptr && d_tgt_items && d_out,
               "lk_bias_score_ragged: null pointer");
    LK_REQUIRE(!d_user_add || d_user_bias, "lk_bias_score_ragged: user flags without user biases");
    hipStream_t st = lk::as_stream(stream);
    const int64_t nb = (n_entries + 255) / 256;
    LK_REQUIRE(nb <= (int64_t)INT32_MAX, "lk_bias_score_ragged: too many entries");
    hipLaunchKernelGGL(lk::bias_score_ragged_kernel, dim3((unsigned)nb), dim3(256), 0, st,
                       n_queries, d_tgt_ptr, d_tgt_items, n_entries, n_items, (float)global_bias,
                       d_item_biases, d_user_bias, d_user_add, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
