// bmf_batch.hip -- `BiasedMFScorer.__call__` (the explicit-feedback ALS model) for a BATCH of
// queries, gfx950: what the per-query path does on the host around its one-row solve and its
// one-row lk_score_dense (lkpy_amd/als.py; src/lenskit/als/_common.py:133-175,
// _explicit.py:55-91, basic/bias.py:166-241) is here, operation for operation.
//
//   bmf_residual_rows_kernel  the fold-in's input: the query's training row (read straight from
//                             the training matrix by user number) with the bias model taken out,
//                             r_j - ((f32(mu) + b_i) + f32(ub)) in float32, and ub itself as the
//                             float64 the host carries to `finalize_scores`.  ub is the sum of
//                             bias_sum.h (NumPy's pairwise order).  One wave per query.
//   bmf_finish_panel_kernel   `finalize_scores` in place on a [rows x items] panel of
//                             lk_score_dense: one read and one write of the panel, 16 bytes per
//                             lane.  bmf_strike_kernel then sets each row's history items to NaN
//                             (a scatter of one thread per history entry: a search per panel
//                             element would put the streaming kernel's loop behind a dependent
//                             load).
//   bmf_finish_pairs_kernel   the same finish for ragged (query, target) lists, the dot product
//                             gathered from the panel.  One thread per entry.
//   bmf_finish_ragged_kernel  the same finish where the dot products are a ragged array already
//                             (lk_score_candidates: no panel).  One thread per entry.
//
// The finish arithmetic is `bmf_finish` and nowhere else.  A row's mode says which branch of
// `__call__` it took, and with it the precision of the sum (include/lkamd.h).
#include "bias_sum.h"
#include "common.h"

// The host sums are plain adds; nothing may be fused.
#pragma clang fp contract(off)

namespace lk {
namespace {

// One score of `finalize_scores`: `dot` is the entry of lk_score_dense, `gb` = f32(mu) + b_i.
//   fold-in row: the host adds a float64 user bias to the float32 biases, and that float64 array
//                to the float32 scores (NEP 50): (double)dot + ((double)gb + ub), rounded once;
//   stored row:  the user bias is the model's float32 value: dot + (gb + ub) in float32.
__device__ __forceinline__ float bmf_finish(float dot, float gb, int mode, double ub)
{
    if (mode == LK_BMF_FOLD) return (float)((double)dot + ((double)gb + ub));
    if (mode == LK_BMF_STORED) return dot + (gb + (float)ub);
    return __builtin_nanf("");
}

template <typename IT>
__global__ __launch_bounds__(WAVE) void bmf_residual_rows_kernel(
    const IT *__restrict__ indptr, UoffSrc src, int64_t n_users, int64_t n_queries,
    const int32_t *__restrict__ user_nums, const int64_t *__restrict__ out_ptr, double damping,
    double *__restrict__ out_ub, int32_t *__restrict__ out_indices, float *__restrict__ out_values)
{
    __shared__ BlockTree tree;
    __shared__ double ub_all;
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= n_queries) return;
    const int32_t u = user_nums[q];
    if (u < 0 || u >= n_users) {  // no row asked for: nothing to write
        if (lane == 0) out_ub[q] = 0.0;
        return;
    }
    const int64_t s = (int64_t)indptr[u];
    int64_t n = (int64_t)indptr[u + 1] - s;
    const double ub = row_user_bias(src, s, n, damping, tree);
    if (lane == 0) {
        out_ub[q] = ub;
        ub_all = ub;
    }
    __syncthreads();
    const float ub32 = (float)ub_all;  // `scores += np.float32(user_bias)`
    const float g32 = (float)src.global_bias;  // np.full(n, mu, float32)
    const int64_t o = out_ptr[q];
    const int64_t room = out_ptr[q + 1] - o;  // (the host's prefix sums: never write past them)
    if (n > room) n = room;
    for (int64_t j = lane; j < n; j += WAVE) {
        const int32_t c = src.indices[s + j];
        float b = g32;
        if (c >= 0 && c < src.n_items) b = b + src.item_biases[c];
        b = b + ub32;
        out_indices[o + j] = c;
        out_values[o + j] = src.values[s + j] - b;
    }
}

constexpr int FP_BLOCK = 256;
constexpr int FP_VEC = 4;  // floats per lane and step: one 16-byte load and store

// four floats from an address that is only 4-byte aligned (the item biases under an unaligned
// row): global memory takes the 16-byte load at any dword address
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

// Row r of the panel starts at element r * ld, which is 16-byte aligned only where r * ld is a
// multiple of four: the row's vectors are laid from the aligned address at or below its start,
// vector i covering columns 4 i - (r * ld) % 4 .. + 3, and a vector that sticks out of the row
// at either end goes element by element.  blockIdx.y strides the rows, blockIdx.x the row's tiles
// of FP_BLOCK vectors.
__global__ __launch_bounds__(FP_BLOCK) void bmf_finish_panel_kernel(
    float *__restrict__ panel, int64_t n_rows, int64_t n_items, int64_t ld,
    const uint8_t *__restrict__ mode, const double *__restrict__ ub, float g32,
    const float *__restrict__ item_biases, int64_t tiles_per_row)
{
    for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const int64_t base = r * ld;
        const int m = mode[r];
        const double u = ub[r];
        float *row = panel + base;
        const int64_t lead = base & (FP_VEC - 1);
        for (int64_t t = blockIdx.x; t < tiles_per_row; t += gridDim.x) {
            const int64_t c0 = (t * FP_BLOCK + threadIdx.x) * FP_VEC - lead;
            if (c0 >= n_items) break;  // (the columns only grow with t)
            if (c0 >= 0 && c0 + FP_VEC <= n_items) {
                f32x4 v = *reinterpret_cast<const f32x4 *>(row + c0);
                const f32x4_u b = *reinterpret_cast<const f32x4_u *>(item_biases + c0);
#pragma unroll
                for (int k = 0; k < FP_VEC; ++k) v[k] = bmf_finish(v[k], g32 + b[k], m, u);
                *reinterpret_cast<f32x4 *>(row + c0) = v;
            } else {
                for (int k = 0; k < FP_VEC; ++k) {
                    const int64_t c = c0 + k;
                    if (c >= 0 && c < n_items)
                        row[c] = bmf_finish(row[c], g32 + item_biases[c], m, u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(WAVE) void bmf_strike_kernel(
    float *__restrict__ panel, int64_t n_rows, int64_t n_items, int64_t ld,
    const int64_t *__restrict__ strike_ptr, const int32_t *__restrict__ strike_items)
{
    const int64_t r = blockIdx.x;
    if (r >= n_rows) return;
    const int64_t lo = strike_ptr[r], hi = strike_ptr[r + 1];
    for (int64_t e = lo + threadIdx.x; e < hi; e += WAVE) {
        const int32_t c = strike_items[e];
        if (c >= 0 && c < n_items) panel[r * ld + c] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void bmf_finish_pairs_kernel(
    const float *__restrict__ panel, int64_t n_rows, int64_t n_items, int64_t ld,
    const uint8_t *__restrict__ mode, const double *__restrict__ ub, float g32,
    const float *__restrict__ item_biases, const int64_t *__restrict__ tgt_ptr,
    const int32_t *__restrict__ tgt_items, int64_t first, int64_t n_entries,
    float *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_entries) return;
    const int64_t e = first + k;
    // the entry's row: the last r with tgt_ptr[r] <= e (empty lists hold no entries)
    int64_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (tgt_ptr[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    const int32_t t = tgt_items[e];
    float s = __builtin_nanf("");  // an unknown item: `item_scores` leaves NaN
    if (t >= 0 && t < n_items)
        s = bmf_finish(panel[lo * ld + t], g32 + item_biases[t], mode[lo], ub[lo]);
    out[e] = s;
}

__global__ __launch_bounds__(256) void bmf_finish_ragged_kernel(
    const float *dots, int64_t n_rows, int64_t n_items, const uint8_t *__restrict__ mode,
    const double *__restrict__ ub, float g32, const float *__restrict__ item_biases,
    const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items, int64_t total,
    float *out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    // the entry's row: the last r with tgt_ptr[r] <= e (empty lists hold no entries)
    int64_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (tgt_ptr[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    const int32_t t = tgt_items[e];
    float s = __builtin_nanf("");  // an unknown item: `item_scores` leaves NaN
    if (t >= 0 && t < n_items) s = bmf_finish(dots[e], g32 + item_biases[t], mode[lo], ub[lo]);
    out[e] = s;
}

}  // namespace
}  // namespace lk

extern "C" int lk_bmf_residual_rows(const void *d_indptr, int indptr_is_64,
                                    const int32_t *d_indices, const float *d_values,
                                    int64_t n_users, int64_t n_items, int64_t n_queries,
                                    const int32_t *d_user_nums, const int64_t *d_out_ptr,
                                    double global_bias, const float *d_item_biases,
                                    double damping_user, double *d_out_ub,
                                    int32_t *d_out_indices, float *d_out_values, void *stream)
{
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_queries >= 0,
               "lk_bmf_residual_rows: negative size");
    if (n_queries == 0) return LK_OK;
    LK_REQUIRE(n_queries <= (int64_t)INT32_MAX, "lk_bmf_residual_rows: too many queries");
    LK_REQUIRE(d_indptr && d_indices && d_values && d_user_nums && d_out_ptr && d_item_biases &&
                   d_out_ub && d_out_indices && d_out_values,
               "lk_bmf_residual_rows: null pointer");
    hipStream_t st = lk::as_stream(stream);
    const lk::UoffSrc src{d_indices, d_values, d_item_biases, n_items, global_bias};
    const dim3 grid((unsigned)n_queries), block(lk::WAVE);
    if (indptr_is_64)
        hipLaunchKernelGGL(lk::bmf_residual_rows_kernel<int64_t>, grid, block, 0, st,
                           static_cast<const int64_t *>(d_indptr), src, n_users, n_queries,
                           d_user_nums, d_out_ptr, damping_user, d_out_ub, d_out_indices,
                           d_out_values);
    else
        hipLaunchKernelGGL(lk::bmf_residual_rows_kernel<int32_t>, grid, block, 0, st,
                           static_cast<const int32_t *>(d_indptr), src, n_users, n_queries,
                           d_user_nums, d_out_ptr, damping_user, d_out_ub, d_out_indices,
                           d_out_values);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_bmf_finish_panel(float *d_panel, int64_t n_rows, int64_t n_items, int64_t ld,
                                   const uint8_t *d_mode, const double *d_ub, double global_bias,
                                   const float *d_item_biases, const int64_t *d_strike_ptr,
                                   const int32_t *d_strike_items, void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n_items >= 0 && ld >= n_items, "lk_bmf_finish_panel: bad shape");
    if (n_rows == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_panel && d_mode && d_ub && d_item_biases, "lk_bmf_finish_panel: null pointer");
    LK_REQUIRE(!d_strike_ptr || d_strike_items, "lk_bmf_finish_panel: offsets without items");
    LK_REQUIRE((reinterpret_cast<uintptr_t>(d_panel) & 15) == 0,
               "lk_bmf_finish_panel: the panel must be 16-byte aligned");
    LK_REQUIRE(n_rows <= (int64_t)INT32_MAX, "lk_bmf_finish_panel: too many rows");
    hipStream_t st = lk::as_stream(stream);
    // vectors per row: up to three columns of lead before the first aligned address
    const int64_t vecs = (n_items + (lk::FP_VEC - 1) + (lk::FP_VEC - 1)) / lk::FP_VEC;
    const int64_t tiles_per_row = (vecs + lk::FP_BLOCK - 1) / lk::FP_BLOCK;
    // 256 CUs x 16 blocks of 256 threads, the rest by the kernel's two strides
    const int64_t cap = 256 * 16;
    const int64_t gx = tiles_per_row < cap ? tiles_per_row : cap;
    const int64_t gy = n_rows < cap / gx ? n_rows : (cap / gx > 0 ? cap / gx : 1);
    hipLaunchKernelGGL(lk::bmf_finish_panel_kernel, dim3((unsigned)gx, (unsigned)gy),
                       dim3(lk::FP_BLOCK), 0, st, d_panel, n_rows, n_items, ld, d_mode, d_ub,
                       (float)global_bias, d_item_biases, tiles_per_row);
    LK_HIP_CHECK(hipGetLastError());
    if (d_strike_ptr) {
        hipLaunchKernelGGL(lk::bmf_strike_kernel, dim3((unsigned)n_rows), dim3(lk::WAVE), 0, st,
                           d_panel, n_rows, n_items, ld, d_strike_ptr, d_strike_items);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}

extern "C" int lk_bmf_finish_pairs(const float *d_panel, int64_t n_rows, int64_t n_items,
                                   int64_t ld, const uint8_t *d_mode, const double *d_ub,
                                   double global_bias, const float *d_item_biases,
                                   const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                                   int64_t first_entry, int64_t n_entries, float *d_out,
                                   void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n_items >= 0 && ld >= n_items && first_entry >= 0 &&
                   n_entries >= 0,
               "lk_bmf_finish_pairs: bad shape");
    if (n_entries == 0) return LK_OK;
    LK_REQUIRE(n_rows > 0 && d_panel && d_mode && d_ub && d_item_biases && d_tgt_ptr &&
                   d_tgt_items && d_out,
               "lk_bmf_finish_pairs: null pointer");
    hipStream_t st = lk::as_stream(stream);
    const int64_t nb = (n_entries + 255) / 256;
    LK_REQUIRE(nb <= (int64_t)INT32_MAX, "lk_bmf_finish_pairs: too many entries");
    hipLaunchKernelGGL(lk::bmf_finish_pairs_kernel, dim3((unsigned)nb), dim3(256), 0, st, d_panel,
                       n_rows, n_items, ld, d_mode, d_ub, (float)global_bias, d_item_biases,
                       d_tgt_ptr, d_tgt_items, first_entry, n_entries, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_bmf_finish_ragged(const float *d_dots, int64_t n_rows, int64_t n_items,
                                    const uint8_t *d_mode, const double *d_ub, double global_bias,
                                    const float *d_item_biases, const int64_t *d_tgt_ptr,
                                    const int32_t *d_tgt_items, int64_t total, float *d_out,
                                    void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n_items >= 0 && total >= 0, "lk_bmf_finish_ragged: bad shape");
    if (total == 0) return LK_OK;
    LK_REQUIRE(n_rows > 0 && d_dots && d_mode && d_ub && d_item_biases && d_tgt_ptr &&
                   d_tgt_items && d_out,
               "lk_bmf_finish_ragged: null pointer");
    const int64_t nb = (total + 255) / 256;
    LK_REQUIRE(nb <= (int64_t)INT32_MAX, "lk_bmf_finish_ragged: too many entries");
    hipLaunchKernelGGL(lk::bmf_finish_ragged_kernel, dim3((unsigned)nb), dim3(256), 0,
                       lk::as_stream(stream), d_dots, n_rows, n_items, d_mode, d_ub,
                       (float)global_bias, d_item_biases, d_tgt_ptr, d_tgt_items, total, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
