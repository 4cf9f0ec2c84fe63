// uknn_predict.hip -- user-kNN scores for the (query, target) PAIRS of a predict call, gfx950.
//
// uknn_recommend.hip scores every item of a panel of queries; `batch.predict` asks for a ragged
// handful of targets per query.  lk_uknn_score_pairs scores exactly those cells, each the way one
// cell of `uknn_score_panel_kernel` is scored (the reference: `UserKNNScorer.__call__`,
// src/lenskit/knn/user.py:171-262; `user_score_items_*`, src/accel/knn/user_score.rs:21-98;
// `ScoreAccumulator`, accum.rs): the target item's column of the TRANSPOSED centred ratings
// (items x users, users ascending) is walked in stored order, every rater whose similarity to
// the query passes `thr` (a NaN does not, the query's own user never) offers (similarity,
// centred rating) to the cell's own accumulator (knn_accum.h) of max_nbrs + 1 slots, and the
// cell is sum(w * v) / sum(w) + offset[q] (explicit) or sum(w) (implicit) over the
// accumulator's final array order, the product rounded before it is added.
//
// Mapping.  One wave per cell, UQ_WAVES waves per workgroup.  The similarities come user-major
// (sims[user][q]: lk_uknn_sims_panel's panel, the cheaper one to produce -- a cell's gathers are
// then one cache line each, but a predict call reads a few per cent of the panel) or query-major
// (sims[q][user]: lk_csr_rows_dot's layout, all the gathers of a cell in one row of n_users
// floats).  The column is loaded 64 entries at a time, coalesced; lane l gathers the
// similarity of its rater and tests it; a ballot marks the passing lanes, which write their
// (similarity, rating) pairs -- compacted in lane order = ascending user number -- into the
// wave's staging row in LDS; lane 0 offers them one by one to the wave's accumulator.  The
// accumulator's minimum only ever rises once it is Full, so testing a whole chunk against the
// minimum it had BEFORE the chunk drops only entries the sequential walk would drop as well
// (`!(heap && s <= minw)`, accum.rs:108); lane 0 repeats the test against the current minimum.
// Cells are numbered by target entry, so the cells of one query are neighbours; a workgroup
// takes four consecutive cells, and the workgroups are renumbered (xcd_remap) so that those
// which run on one XCD walk one contiguous range of cells: a query's similarities are
// pulled into one L2, not eight.  A cell finds its query by a 64-ary search of the wave over
// the target offsets (three rounds for 262 144 queries).
//
// Where the accumulators live.  An accumulator never holds more than the longest column's
// entries: S = min(max_nbrs, max_col_len) + 1 slots of (w, v), 8 S bytes per wave.
//   S <= 128 (max_nbrs <= UQ_LDS_NBR_MAX = 127): in LDS, 1 KB per wave; with the staging rows a
//       workgroup holds 6 KB, so LDS never limits the waves per CU.
//   above: in a slab of the workspace per resident wave (lk_uknn_score_pairs_workspace_bytes:
//       as many workgroups as UQ_SLAB_BUDGET holds, at most UQ_SLAB_BLOCKS, at least one), the
//       workgroups striding over the cells.  Any max_nbrs an int32 holds is taken.
// No atomics: the same inputs give the same bits.
#include "common.h"
#include "knn_accum.h"

// The reference's sums are plain f32 multiplies and adds: `weight * value` is rounded before it
// is added.
#pragma clang fp contract(off)

namespace lk {

constexpr int UQ_WAVES = 4;                    // waves (= cells in flight) per workgroup
constexpr int UQ_LDS_NBR_MAX = 127;            // (127 + 1) slots x 8 bytes = 1 KB per wave
constexpr int UQ_LDS_SLOTS = UQ_LDS_NBR_MAX + 1;
constexpr int64_t UQ_SLAB_BLOCKS = 1024;       // resident workgroups of the slab variant, at most
constexpr size_t UQ_SLAB_BUDGET = 512u << 20;  // ... and what their slabs may take together
constexpr int64_t UQ_MAX_GRID = 1 << 20;

static inline int64_t uq_slots(int32_t max_nbrs, int64_t max_col_len)
{
    const int64_t m = max_col_len < (int64_t)max_nbrs ? max_col_len : (int64_t)max_nbrs;
    return (m < 1 ? 1 : m) + 1;
}
static inline int64_t uq_slab_blocks(int64_t slots)
{
    const int64_t fit = (int64_t)(UQ_SLAB_BUDGET / ((size_t)slots * 8 * UQ_WAVES));
    return fit < 1 ? 1 : (fit > UQ_SLAB_BLOCKS ? UQ_SLAB_BLOCKS : fit);
}

// The largest q in [0, n) with ptr[q] <= cell, for ptr[0] <= cell and ptr non-decreasing: the
// wave looks at 64 evenly spaced offsets per round.  Wave-uniform; always inside [0, n).
__device__ __forceinline__ int64_t uq_find_query(const int64_t *__restrict__ ptr, int64_t n,
                                                 int64_t cell, int lane)
{
    int64_t lo = 0;
    while (n > 1) {
        const int64_t step = (n + 63) / 64;
        const int64_t at = lo + (int64_t)lane * step;
        const bool below = lane == 0 || (at < lo + n && ptr[at] <= cell);
        // (the lanes that pass are a prefix; a pointer array that is not sorted still leaves k
        // among the lanes inside the range)
        const unsigned long long m = __ballot(below);
        const int k = 63 - __builtin_clzll(m);
        const int64_t left = lo + n - (lo + (int64_t)k * step);
        lo += (int64_t)k * step;
        n = left < step ? left : step;
    }
    return lo;
}

// LDS: the waves' accumulators in LDS, else each in its slab of `ws`.  `max_nbrs` is already
// clamped to slots - 1 (a column has no more entries than that: nothing changes).
template <bool LDS>
__global__ __launch_bounds__(UQ_WAVES * 64) void uknn_score_pairs_kernel(
    const int64_t *__restrict__ t_ptr, const int32_t *__restrict__ t_users,
    const float *__restrict__ t_vals, int64_t n_items, int64_t n_users,
    const float *__restrict__ sims, int64_t stride_q, int64_t stride_u, int64_t n_queries,
    const int32_t *__restrict__ self_user, const int64_t *__restrict__ tgt_ptr,
    const int32_t *__restrict__ tgt_items, int64_t entry_lo, int64_t entry_hi, float thr,
    int max_nbrs, int min_nbrs, int64_t slots, const float *__restrict__ offset,
    float *__restrict__ ws, float *__restrict__ out)
{
    __shared__ float uq_acc[LDS ? UQ_WAVES * UQ_LDS_SLOTS * 2 : 1];
    __shared__ float uq_stage[UQ_WAVES * 128];  // per wave: 64 similarities, 64 ratings
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *aw = LDS ? uq_acc + wv * (UQ_LDS_SLOTS * 2)
                    : ws + ((size_t)blockIdx.x * UQ_WAVES + wv) * (size_t)slots * 2;
    float *av = aw + (LDS ? (int64_t)UQ_LDS_SLOTS : slots);
    float *stg = uq_stage + wv * 128;
    const bool explicit_ = t_vals != nullptr;
    const float nanf_ = __builtin_nanf("");
    int64_t c0 = tgt_ptr[0], c1 = tgt_ptr[n_queries];
    if (c0 < entry_lo) c0 = entry_lo;
    if (c1 > entry_hi) c1 = entry_hi;

    const int64_t first = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * UQ_WAVES + wv;
    for (int64_t cell = c0 + first; cell < c1; cell += (int64_t)gridDim.x * UQ_WAVES) {
        const int64_t q = uq_find_query(tgt_ptr, n_queries, cell, lane);
        const int item = tgt_items[cell];
        float score = nanf_;
        if (item >= 0 && item < n_items) {
            const float *srow = sims + q * stride_q;
            const int self = self_user ? self_user[q] : -1;
            const int64_t b = t_ptr[item], e = t_ptr[item + 1];
            // (wave-uniform; lane 0 changes them, the others take its values after each chunk)
            int len = 0, heap = 0;
            float minw = 0.f;  // the heap's minimum once it is Full: most later entries stop here
            int64_t me = b + lane;
            int u = me < e ? t_users[me] : -1;
            float r = (explicit_ && me < e) ? t_vals[me] : 0.f;
            for (int64_t base = b; base < e; base += 64) {
                // the next chunk's entries are on their way while this one is offered
                const int64_t nx = base + 64 + lane;
                const int u_nx = nx < e ? t_users[nx] : -1;
                const float r_nx = (explicit_ && nx < e) ? t_vals[nx] : 0.f;
                // user.py:192-206: the own user's similarity is zero, below every min_sim; a NaN
                // similarity fails the comparison
                const float s = (u >= 0 && u < n_users && u != self)
                                    ? srow[(int64_t)u * stride_u] : nanf_;
                const bool pass = s >= thr && !(heap && s <= minw);
                const unsigned long long m = __ballot(pass);
                if (m != 0ull) {
                    if (pass) {
                        const int at = __builtin_popcountll(m & ((1ull << lane) - 1ull));
                        stg[at] = s;
                        stg[64 + at] = r;
                    }
                    wave_lds_sync();
                    if (lane == 0) {
                        const int cnt = __builtin_popcountll(m);
                        bool hp = heap != 0;
                        for (int i = 0; i < cnt; ++i) {
                            const float si = stg[i];
                            // accum.rs:108: a Full accumulator ignores what is not strictly
                            // greater than its minimum
                            if (!(hp && si <= minw)) {
                                kf_offer<1>(aw, av, len, hp, max_nbrs, si, stg[64 + i]);
                                if (hp) minw = aw[0];
                            }
                        }
                        heap = hp ? 1 : 0;
                    }
                    len = __builtin_amdgcn_readfirstlane(len);
                    heap = __builtin_amdgcn_readfirstlane(heap);
                    minw = __builtin_bit_cast(
                        float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, minw)));
                    wave_lds_sync();  // the staging row is free again
                }
                u = u_nx;
                r = r_nx;
            }
            if (lane == 0 && len >= min_nbrs && len > 0) {
                // total_weight / weighted_sum (accum.rs:121-140): sequential sums in array order
                float tw = 0.f, wsum = 0.f;
                for (int i = 0; i < len; ++i) {
                    const float w = aw[i];
                    tw += w;
                    wsum += w * av[i];
                }
                score = explicit_ ? wsum / tw + (offset ? offset[q] : 0.f) : tw;
            }
        }
        if (lane == 0) out[cell] = score;
    }
}

}  // namespace lk

extern "C" int32_t lk_uknn_score_pairs_lds_max_nbrs(void) { return lk::UQ_LDS_NBR_MAX; }

extern "C" size_t lk_uknn_score_pairs_workspace_bytes(int32_t max_nbrs, int64_t max_col_len)
{
    if (max_nbrs < 1 || max_col_len < 0) return 0;
    const int64_t slots = lk::uq_slots(max_nbrs, max_col_len);
    if (slots - 1 <= lk::UQ_LDS_NBR_MAX) return 0;
    return (size_t)lk::uq_slab_blocks(slots) * lk::UQ_WAVES * (size_t)slots * 8;
}

extern "C" int lk_uknn_score_pairs(const int64_t *d_t_indptr, const int32_t *d_t_users,
                                   const float *d_t_values, int64_t n_items, int64_t n_users,
                                   int64_t max_col_len, const float *d_sims, int64_t ld_sims,
                                   int sims_user_major, int64_t n_queries,
                                   const int32_t *d_self_user,
                                   const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                                   int64_t first_entry, int64_t n_entries, float thr,
                                   int32_t max_nbrs, int32_t min_nbrs, const float *d_offset,
                                   void *d_ws, float *d_out, void *stream)
{
    LK_REQUIRE(max_nbrs >= 1 && min_nbrs >= 1,
               "lk_uknn_score_pairs: max_nbrs/min_nbrs must be >= 1");
    LK_REQUIRE(n_items >= 0 && n_users >= 0 && n_queries >= 0 && max_col_len >= 0 &&
                   ld_sims >= (sims_user_major ? n_queries : n_users) && first_entry >= 0 &&
                   n_entries >= 0,
               "lk_uknn_score_pairs: bad shape");
    if (n_queries == 0 || n_entries == 0) return LK_OK;
    LK_REQUIRE(d_t_indptr && d_sims && d_tgt_ptr && d_tgt_items && d_out,
               "lk_uknn_score_pairs: null pointer");
    hipStream_t st = lk::as_stream(stream);
    const int64_t slots = lk::uq_slots(max_nbrs, max_col_len);
    const int eff_nbrs = (int)(slots - 1 < (int64_t)max_nbrs ? slots - 1 : (int64_t)max_nbrs);
    const int64_t n_blocks = (n_entries + lk::UQ_WAVES - 1) / lk::UQ_WAVES;
    const dim3 block(lk::UQ_WAVES * 64);
    const int64_t stride_q = sims_user_major ? 1 : ld_sims;
    const int64_t stride_u = sims_user_major ? ld_sims : 1;
    if (slots - 1 <= lk::UQ_LDS_NBR_MAX) {
        const int64_t grid = n_blocks < lk::UQ_MAX_GRID ? n_blocks : lk::UQ_MAX_GRID;
        hipLaunchKernelGGL(lk::uknn_score_pairs_kernel<true>, dim3((unsigned)grid), block, 0, st,
                           d_t_indptr, d_t_users, d_t_values, n_items, n_users, d_sims, stride_q,
                           stride_u, n_queries, d_self_user, d_tgt_ptr, d_tgt_items, first_entry,
                           first_entry + n_entries, thr, eff_nbrs, (int)min_nbrs, slots, d_offset,
                           (float *)nullptr, d_out);
    } else {
        LK_REQUIRE(d_ws, "lk_uknn_score_pairs: null workspace");
        const int64_t res = lk::uq_slab_blocks(slots);
        const int64_t grid = n_blocks < res ? n_blocks : res;
        hipLaunchKernelGGL(lk::uknn_score_pairs_kernel<false>, dim3((unsigned)grid), block, 0, st,
                           d_t_indptr, d_t_users, d_t_values, n_items, n_users, d_sims, stride_q,
                           stride_u, n_queries, d_self_user, d_tgt_ptr, d_tgt_items, first_entry,
                           first_entry + n_entries, thr, eff_nbrs, (int)min_nbrs, slots, d_offset,
                           static_cast<float *>(d_ws), d_out);
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
