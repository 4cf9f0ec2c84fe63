// uknn_recommend.hip -- user-kNN for whole PANELS of queries, every item scored, gfx950.
//
// The reference scores one query per call (`UserKNNScorer.__call__`, src/lenskit/knn/user.py:171-255;
// `user_score_items_*`, src/accel/knn/user_score.rs:21-98): it walks the query's neighbours in
// ascending user number and scatters each neighbour's rating row into per-item
// `ScoreAccumulator`s (accum.rs).  Seen from ONE item i, that accumulator receives exactly the
// raters of i, in ascending user number, of which those count whose similarity to the query
// passes `min_sim`; each offers (similarity, centred rating).  So with the TRANSPOSED rating
// matrix (items x users, users ascending in a row: `lk_csr_transpose` is stable) every
// (query, item) cell is a gather with a private accumulator: no scatter, no slab reset, no
// neighbour compaction, no barrier.  Three kernels make a panel:
//
// lk_uknn_query_panel   X[item][q]: the dense query vectors of a panel of histories
//                       (rating - centre, or 1.0), item-major as lk_csr_rows_dot reads them.
//                       A wave per query; a repeated item keeps its LAST occurrence.
// lk_uknn_sims_panel    sims[user][q] = <user_vectors[user], X[:, q]>: `csr_rows_dot_kernel`
//                       (iknn_score.hip) with the output user-major -- the 64 queries of a lane
//                       block contiguous -- and the query's own user written as +0.0
//                       (user.py:192-194).  The same fmaf chain over the stored row: the same bits.
// lk_uknn_score_panel   out[q][item]: one wave per (item column, block of 64 queries), lane =
//                       query.  The column's entries are loaded 64 at a time and broadcast;
//                       every step is one coalesced 256-byte read of sims[user][q0 .. q0 + 63].
//                       A lane whose similarity passes `thr` (NaN does not) offers (similarity,
//                       rating) to its accumulator -- knn_accum.h, the reference's, step for
//                       step -- of max_nbrs + 1 (w, v) pairs, the lanes' accumulators
//                       interleaved (element i of lane l at [i * 64 + l]: no LDS bank conflict,
//                       coalesced in global memory).  Then sum(w * v) / sum(w) + offset[q]
//                       (explicit) or sum(w) (implicit) in final array order, the product
//                       rounded before it is added; fewer than min_nbrs entries: NaN.  A second
//                       small kernel strikes the cells of the queries' own items.
//
// Where the accumulators live.  No accumulator ever holds more than the longest column's entries,
// so it has S = min(max_nbrs, max_col_len) + 1 slots, 512 S bytes per wave.
//   S <= 128 (max_nbrs <= UP_LDS_NBR_MAX = 127, 64 KB): in LDS, one wave per workgroup, one
//       workgroup per task (15.9 KB at the default max_nbrs = 30: ten waves per CU).
//   above: in a slab of the workspace per resident wave (lk_uknn_score_panel_workspace_bytes:
//       as many waves as UP_SLAB_BUDGET holds, at most UP_SLAB_WAVES, at least one), the waves
//       striding over the tasks.  Any max_nbrs an int32 holds is taken.
// Tasks are numbered item-major in `d_item_order` (the caller's: heaviest column first), so the
// long columns start first and the tail of the launch is short ones.
#include "common.h"
#include "knn_accum.h"

// The reference's sums are plain f32 multiplies and adds: `weight * value` is rounded before it
// is added (the fmaf of the sims kernel is written out and not affected).
#pragma clang fp contract(off)

namespace lk {

constexpr int UP_LDS_NBR_MAX = 127;            // (127 + 1) slots x 64 lanes x 8 bytes = 64 KB
constexpr int UP_SLAB_WAVES = 2048;            // resident waves of the slab variant, at most
constexpr size_t UP_SLAB_BUDGET = 512u << 20;  // ... and what their slabs may take together
constexpr int64_t UP_MAX_GRID = 1 << 20;
constexpr int UP_PF = 8;                       // similarities a lane has in flight

static inline int64_t up_slots(int32_t max_nbrs, int64_t max_col_len)
{
    const int64_t m = max_col_len < (int64_t)max_nbrs ? max_col_len : (int64_t)max_nbrs;
    return (m < 1 ? 1 : m) + 1;
}
static inline int64_t up_slab_waves(int64_t slots)
{
    const int64_t fit = (int64_t)(UP_SLAB_BUDGET / ((size_t)slots * 512));
    return fit < 1 ? 1 : (fit > UP_SLAB_WAVES ? UP_SLAB_WAVES : fit);
}

// ---- X[item][q] ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uknn_query_panel_kernel(
    const int64_t *__restrict__ h_ptr, const int32_t *__restrict__ h_items,
    const float *__restrict__ h_rates, const float *__restrict__ centre, int64_t n_queries,
    int64_t n_items, float *__restrict__ x, int64_t ld_x)
{
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_queries) return;
    const int lane = threadIdx.x & 63;
    const int64_t b = h_ptr[q], e = h_ptr[q + 1];
    const float c = h_rates ? centre[q] : 0.f;
    for (int64_t base = b; base < e; base += 64) {
        // stores of one wave to one address land in program order once the earlier ones are
        // acknowledged: a later chunk's repeat of an item overwrites the earlier chunk's
        if (base > b) __threadfence();
        const int64_t me = base + lane;
        const int it = me < e ? h_items[me] : -1;
        const int n = (e - base) < 64 ? (int)(e - base) : 64;
        // within the chunk the LAST occurrence of an item writes (`ratings[nos[ok]] = ...`)
        bool last = it >= 0 && it < n_items;
        for (int j = 1; j < n; ++j) {
            const int itj = __builtin_amdgcn_readlane(it, j);
            if (j > lane && itj == it) last = false;
        }
        if (last) x[(int64_t)it * ld_x + q] = h_rates ? h_rates[me] - c : 1.0f;
    }
}

// ---- sims[user][q]: csr_rows_dot_kernel with the output user-major and the self entry zero -----
template <bool IS64>
__global__ __launch_bounds__(256) void uknn_sims_panel_kernel(
    const typename IndPtr<IS64>::type *__restrict__ ptr, const int32_t *__restrict__ idx,
    const float *__restrict__ val, int64_t n_rows, const float *__restrict__ x, int64_t ld_x,
    int64_t n_queries, const int32_t *__restrict__ self_user, float *__restrict__ out,
    int64_t ld_out)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t b = ptr[row], e = ptr[row + 1];
    // (csr_rows_dot_kernel walks the query blocks in a loop; here they are the grid's y: a
    // small model -- few rows -- still fills the device.  A (row, query) chain is the same.)
    const int64_t q = (int64_t)blockIdx.y * 64 + lane;
    float acc = 0.f;
    for (int64_t base = b; base < e; base += 64) {
        // 64 entries of the row per coalesced load, then broadcast one by one
        const int64_t me = base + lane;
        const int it = me < e ? idx[me] : 0;
        const float v = me < e ? val[me] : 0.f;
        const int n = (e - base) < 64 ? (int)(e - base) : 64;
        // (UP_PF loads in flight, then the products in stored order: the chain is unchanged)
        for (int j0 = 0; j0 < n; j0 += UP_PF) {
            float xv[UP_PF];
#pragma unroll
            for (int k = 0; k < UP_PF; ++k) {
                const int itj = __builtin_amdgcn_readlane(it, (j0 + k) & 63);
                xv[k] = (q < n_queries && j0 + k < n) ? x[(int64_t)itj * ld_x + q] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < UP_PF; ++k)
                if (j0 + k < n) acc = fmaf(bcast(v, (j0 + k) & 63), xv[k], acc);
        }
    }
    if (q < n_queries) {
        if (self_user && (int64_t)self_user[q] == row) acc = 0.f;  // user.py:192-194
        out[row * ld_out + q] = acc;
    }
}

// ---- out[q][item] ------------------------------------------------------------------------------
// LDS: the wave's accumulators in (dynamic) LDS, else in its slab of `ws`.  `max_nbrs` here is
// already clamped to slots - 1 (a column has no more entries than that: nothing changes).
template <bool LDS>
__global__ __launch_bounds__(64) void uknn_score_panel_kernel(
    const int64_t *__restrict__ t_ptr, const int32_t *__restrict__ t_users,
    const float *__restrict__ t_vals, int64_t n_items, int64_t n_users,
    const int32_t *__restrict__ item_order, const float *__restrict__ sims, int64_t ld_s,
    int64_t n_queries, float thr, int max_nbrs, int min_nbrs, int64_t slots,
    const float *__restrict__ offset, float *__restrict__ ws, float *__restrict__ out,
    int64_t ld_out)
{
    extern __shared__ float up_lds[];
    const int lane = threadIdx.x;
    float *aw = (LDS ? up_lds : ws + (size_t)blockIdx.x * (size_t)slots * 128) + lane;
    float *av = aw + (size_t)slots * 64;
    const bool explicit_ = t_vals != nullptr;
    const int64_t n_qb = (n_queries + 63) / 64;
    const int64_t n_tasks = n_items * n_qb;
    const float nanf_ = __builtin_nanf("");

    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t slot = task / n_qb;
        const int64_t item = item_order ? (int64_t)item_order[slot] : slot;
        if (item < 0 || item >= n_items) continue;
        const int64_t q = (task - slot * n_qb) * 64 + lane;
        const bool live = q < n_queries;
        const float *srow = sims + (live ? q : 0);
        const int64_t b = t_ptr[item], e = t_ptr[item + 1];
        int len = 0;
        bool heap = false;
        float minw = 0.f;  // the heap's minimum once it is Full: most later entries stop here
        for (int64_t base = b; base < e; base += 64) {
            const int64_t me = base + lane;
            int u = me < e ? t_users[me] : -1;
            if (u >= n_users) u = -1;
            const float r = (explicit_ && me < e) ? t_vals[me] : 0.f;
            const int n = (e - base) < 64 ? (int)(e - base) : 64;
            for (int j0 = 0; j0 < n; j0 += UP_PF) {
                float s[UP_PF];
#pragma unroll
                for (int k = 0; k < UP_PF; ++k) {
                    // (lanes past n hold -1: the step loads nothing)
                    const int uj = __builtin_amdgcn_readlane(u, (j0 + k) & 63);
                    s[k] = (live && j0 + k < n && uj >= 0) ? srow[(int64_t)uj * ld_s] : nanf_;
                }
#pragma unroll
                for (int k = 0; k < UP_PF; ++k) {
                    const float rj = bcast(r, (j0 + k) & 63);
                    // user.py:206: a NaN similarity fails the comparison; accum.rs:108: a Full
                    // accumulator ignores what is not strictly greater than its minimum
                    if (s[k] >= thr && !(heap && s[k] <= minw)) {
                        kf_offer<64>(aw, av, len, heap, max_nbrs, s[k], rj);
                        if (heap) minw = aw[0];
                    }
                }
            }
        }
        float score = nanf_;
        if (len >= min_nbrs && len > 0) {
            // total_weight / weighted_sum (accum.rs:121-140): sequential sums in array order
            float tw = 0.f, wsum = 0.f;
            for (int i = 0; i < len; ++i) {
                const float w = aw[i * 64];
                tw += w;
                wsum += w * av[i * 64];
            }
            score = explicit_ ? wsum / tw + (offset ? offset[q] : 0.f) : tw;
        }
        if (live) out[q * ld_out + item] = score;
    }
}

// the queries' own items NaN (bit 0), the whole row of a query without a known item NaN (bit 1)
__global__ __launch_bounds__(256) void uknn_strike_kernel(
    const int64_t *__restrict__ h_ptr, const int32_t *__restrict__ h_items, int64_t n_items,
    int flags, float *__restrict__ out, int64_t ld_out)
{
    const int64_t q = blockIdx.x;
    const int64_t b = h_ptr[q], e = h_ptr[q + 1];
    const float nanf_ = __builtin_nanf("");
    int known = 0;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) {
        const int it = h_items[i];
        if (it < 0 || it >= n_items) continue;
        known = 1;
        if (flags & 1) out[q * ld_out + it] = nanf_;
    }
    if ((flags & 2) && !__syncthreads_or(known))
        for (int64_t i = threadIdx.x; i < n_items; i += 256) out[q * ld_out + i] = nanf_;
}

}  // namespace lk

extern "C" int lk_uknn_query_panel(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                                   const float *d_hist_ratings, const float *d_centre,
                                   int64_t n_queries, int64_t n_items, float *d_x, int64_t ld_x,
                                   void *stream)
{
    LK_REQUIRE(n_queries >= 0 && n_items >= 0 && ld_x >= n_queries,
               "lk_uknn_query_panel: bad shape");
    if (n_queries == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_hist_ptr && d_x && (!d_hist_ratings || d_centre),
               "lk_uknn_query_panel: null pointer");
    hipStream_t st = lk::as_stream(stream);
    LK_HIP_CHECK(hipMemset2DAsync(d_x, (size_t)ld_x * sizeof(float), 0,
                                  (size_t)n_queries * sizeof(float), (size_t)n_items, st));
    hipLaunchKernelGGL(lk::uknn_query_panel_kernel, dim3((unsigned)((n_queries + 3) / 4)),
                       dim3(256), 0, st, d_hist_ptr, d_hist_items, d_hist_ratings, d_centre,
                       n_queries, n_items, d_x, ld_x);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_uknn_sims_panel(const void *d_indptr, int indptr_is_64,
                                  const int32_t *d_indices, const float *d_values,
                                  int64_t n_users, const float *d_x, int64_t ld_x,
                                  int64_t n_queries, const int32_t *d_self_user, float *d_out,
                                  int64_t ld_out, void *stream)
{
    LK_REQUIRE(n_users >= 0 && n_queries >= 0 && ld_x >= n_queries && ld_out >= n_queries,
               "lk_uknn_sims_panel: bad shape");
    if (n_users == 0 || n_queries == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_x && d_out, "lk_uknn_sims_panel: null pointer");
    LK_REQUIRE(n_queries <= 64 * 65535, "lk_uknn_sims_panel: at most 4 193 280 queries per call");
    hipStream_t st = lk::as_stream(stream);
    const dim3 grid((unsigned)((n_users + 3) / 4), (unsigned)((n_queries + 63) / 64)), block(256);
    if (indptr_is_64)
        hipLaunchKernelGGL(lk::uknn_sims_panel_kernel<true>, grid, block, 0, st,
                           static_cast<const int64_t *>(d_indptr), d_indices, d_values, n_users,
                           d_x, ld_x, n_queries, d_self_user, d_out, ld_out);
    else
        hipLaunchKernelGGL(lk::uknn_sims_panel_kernel<false>, grid, block, 0, st,
                           static_cast<const int32_t *>(d_indptr), d_indices, d_values, n_users,
                           d_x, ld_x, n_queries, d_self_user, d_out, ld_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int32_t lk_uknn_score_panel_lds_max_nbrs(void) { return lk::UP_LDS_NBR_MAX; }

extern "C" size_t lk_uknn_score_panel_workspace_bytes(int32_t max_nbrs, int64_t max_col_len)
{
    if (max_nbrs < 1 || max_col_len < 0) return 0;
    const int64_t slots = lk::up_slots(max_nbrs, max_col_len);
    if (slots - 1 <= lk::UP_LDS_NBR_MAX) return 0;
    return (size_t)lk::up_slab_waves(slots) * (size_t)slots * 512;
}

extern "C" int lk_uknn_score_panel(const int64_t *d_t_indptr, const int32_t *d_t_users,
                                   const float *d_t_values, int64_t n_items, int64_t n_users,
                                   int64_t max_col_len, const int32_t *d_item_order,
                                   const float *d_sims, int64_t ld_sims, int64_t n_queries,
                                   float thr, int32_t max_nbrs, int32_t min_nbrs,
                                   const float *d_offset, const int64_t *d_hist_ptr,
                                   const int32_t *d_hist_items, int mark_history, void *d_ws,
                                   float *d_out, int64_t ld_out, void *stream)
{
    LK_REQUIRE(max_nbrs >= 1 && min_nbrs >= 1, "lk_uknn_score_panel: max_nbrs/min_nbrs must be >= 1");
    LK_REQUIRE(n_items >= 0 && n_users >= 0 && n_queries >= 0 && max_col_len >= 0 &&
                   ld_sims >= n_queries && ld_out >= n_items,
               "lk_uknn_score_panel: bad shape");
    if (n_queries == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_t_indptr && d_sims && d_out, "lk_uknn_score_panel: null pointer");
    LK_REQUIRE(!(mark_history & 3) || d_hist_ptr, "lk_uknn_score_panel: no history to mark");
    LK_REQUIRE(n_queries <= 0x7fffffff, "lk_uknn_score_panel: too many queries");
    hipStream_t st = lk::as_stream(stream);
    const int64_t slots = lk::up_slots(max_nbrs, max_col_len);
    const int eff_nbrs = (int)(slots - 1 < (int64_t)max_nbrs ? slots - 1 : (int64_t)max_nbrs);
    const int64_t n_tasks = n_items * ((n_queries + 63) / 64);
    if (slots - 1 <= lk::UP_LDS_NBR_MAX) {
        const int64_t grid = n_tasks < lk::UP_MAX_GRID ? n_tasks : lk::UP_MAX_GRID;
        hipLaunchKernelGGL(lk::uknn_score_panel_kernel<true>, dim3((unsigned)grid), dim3(64),
                           (size_t)slots * 512, st, d_t_indptr, d_t_users, d_t_values, n_items,
                           n_users, d_item_order, d_sims, ld_sims, n_queries, thr, eff_nbrs,
                           (int)min_nbrs, slots, d_offset, (float *)nullptr, d_out, ld_out);
    } else {
        LK_REQUIRE(d_ws, "lk_uknn_score_panel: null workspace");
        const int64_t waves = lk::up_slab_waves(slots);
        const int64_t grid = n_tasks < waves ? n_tasks : waves;
        hipLaunchKernelGGL(lk::uknn_score_panel_kernel<false>, dim3((unsigned)grid), dim3(64), 0,
                           st, d_t_indptr, d_t_users, d_t_values, n_items, n_users, d_item_order,
                           d_sims, ld_sims, n_queries, thr, eff_nbrs, (int)min_nbrs, slots,
                           d_offset, static_cast<float *>(d_ws), d_out, ld_out);
    }
    LK_HIP_CHECK(hipGetLastError());
    if (mark_history & 3) {
        hipLaunchKernelGGL(lk::uknn_strike_kernel, dim3((unsigned)n_queries), dim3(256), 0, st,
                           d_hist_ptr, d_hist_items, n_items, mark_history, d_out, ld_out);
        LK_HIP_CHECK(hipGetLastError());
    }
    return LK_OK;
}
