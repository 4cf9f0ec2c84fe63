// assoc.hip -- association rules (conditional probability, lift, damped "biased lift") on the
// device: the training epilogue that turns co-occurrence counts into scores, and the batched
// scorer that reduces the reference items' rows by mean or max.
//
// Replaces the in-place NumPy scaling of `AssociationScorer.train` (src/lenskit/knn/
// association.py:110-124) and the densify-and-reduce of `AssociationScorer.__call__`
// (association.py:149-155).  The co-occurrence counts themselves are the similarity build on
// unit values (lk_iknn_build_*, threshold 0.5), as for EASE and `fast_col_cooc`.
//
// SCALING.  One streaming pass over the CSR the build left in HBM, in place, a workgroup per row
// (grid-stride): NumPy divides the float32 counts by an `int32 + float` array, i.e. in float64 and
// rounds once to float32; the lift's `*= n_groups` is a float32 multiply by float32(n_groups).
//
// SCORING.  A task is (query, window of item columns); the window's accumulators live in LDS.
// Each of the workgroup's four waves owns a contiguous slice of the window and walks ALL the
// query's reference rows for that slice BY ITSELF, one row after the other in reference-item
// order: it finds where its slice starts and ends in the (column-sorted) row by two 64-ary
// searches run in lockstep -- every lane probes, a ballot counts the probes below the bound, at
// most three rounds for rows of up to 64^3 entries -- and then adds (or maxes) the entries
// between, 64 to the instruction, the loads of the next four instructions already in flight.  A row
// names a column once, so the lanes of one instruction never meet on a cell; nothing but the
// owning wave ever touches a cell, so the additions of a cell happen in
// reference-item order with no workgroup barrier and no atomic; the hardware keeps one wave's LDS
// operations in order and a wavefront fence between two rows keeps the compiler from reordering
// them.  The next row's (item, begin, end) are fetched while the current row is walked.  The
// epilogue strikes the query's own items in LDS and streams the slice out once, coalesced:
// float32(double(sum) / double(m)) for the mean, the cell itself for the max.
// A query's bits do not depend on the batch it is scored in: the task sees its own query only.
#include "common.h"

namespace lk {

// Accumulator cells of one workgroup: 32 KiB of the CU's 160 KiB LDS, so five workgroups = 20
// waves are resident per CU; the windows of one query are made equally wide (multiples of 64).
constexpr int ASSOC_WINDOW = 8192;
constexpr int ASSOC_THREADS = 256;
constexpr int ASSOC_WAVES = ASSOC_THREADS / WAVE;

__global__ __launch_bounds__(256) void assoc_scale_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    float *__restrict__ values, const int32_t *__restrict__ item_counts, int64_t n_items,
    float n_groups, int lift, double damping)
{
    for (int64_t r = blockIdx.x; r < n_items; r += gridDim.x) {
        const int64_t b = indptr[r], e = indptr[r + 1];
        if (b == e) continue;
        const double dr = (double)item_counts[r] + damping;
        for (int64_t k = b + threadIdx.x; k < e; k += 256) {
            float v = (float)((double)values[k] / dr);
            if (lift) {
                v = v * n_groups;
                v = (float)((double)v / ((double)item_counts[indices[k]] + damping));
            }
            values[k] = v;
        }
    }
}

// p0 / p1: the first positions in the sorted row idx[lo, hi) whose column is >= t0 / >= t1 (hi if
// none).  Two 64-ary searches in lockstep -- every lane probes once for each target, a ballot
// counts the probes below it (they lead: the row is sorted) -- so a round costs one memory
// latency for both, and rows of up to 64^3 entries take at most three rounds.  Wave-uniform
// arguments and results; all 64 lanes take part.
__device__ __forceinline__ void wave_bounds(const int32_t *__restrict__ idx, int64_t lo,
                                            int64_t hi, int32_t t0, int32_t t1, int64_t &p0,
                                            int64_t &p1)
{
    const int lane = lane_id();
    int64_t lo0 = lo, hi0 = hi, lo1 = lo, hi1 = hi;
    while (lo0 < hi0 || lo1 < hi1) {
        const int64_t st0 = (hi0 - lo0 + 63) >> 6, st1 = (hi1 - lo1 + 63) >> 6;
        const int64_t q0 = lo0 + (int64_t)lane * st0, q1 = lo1 + (int64_t)lane * st1;
        const int32_t a = q0 < hi0 ? idx[q0] : INT32_MAX;
        const int32_t b = q1 < hi1 ? idx[q1] : INT32_MAX;
        const int c0 = __popcll(__ballot(a < t0)), c1 = __popcll(__ballot(b < t1));
        if (c0 == 0) {
            hi0 = lo0;  // (also the state of a finished search: it stays finished)
        } else {
            const int64_t nh = lo0 + (int64_t)c0 * st0;
            lo0 += (int64_t)(c0 - 1) * st0 + 1;
            hi0 = nh < hi0 ? nh : hi0;
        }
        if (c1 == 0) {
            hi1 = lo1;
        } else {
            const int64_t nh = lo1 + (int64_t)c1 * st1;
            lo1 += (int64_t)(c1 - 1) * st1 + 1;
            hi1 = nh < hi1 ? nh : hi1;
        }
    }
    p0 = lo0;
    p1 = lo1;
}

template <bool MAX>
__global__ __launch_bounds__(256) void assoc_score_kernel(
    const int64_t *__restrict__ ref_ptr, const int32_t *__restrict__ ref_items,
    const int64_t *__restrict__ s_ptr, const int32_t *__restrict__ s_idx,
    const float *__restrict__ s_val, int64_t n_items, int32_t n_win, int32_t win_w,
    float *__restrict__ out, int64_t ld_out, int mark)
{
    __shared__ float acc[ASSOC_WINDOW];
    const int64_t q = blockIdx.x / (unsigned)n_win;
    const int32_t win = (int32_t)(blockIdx.x % (unsigned)n_win);
    const int64_t w0 = (int64_t)win * win_w;
    const int64_t w1 = w0 + win_w < n_items ? w0 + win_w : n_items;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    // this wave's slice [s0, s1) of the window: a quarter, rounded up to whole instructions
    const int64_t sw = (((w1 - w0) + ASSOC_WAVES - 1) / ASSOC_WAVES + 63) & ~(int64_t)63;
    const int64_t s0 = w0 + wave * sw;
    const int64_t s1 = s0 + sw < w1 ? s0 + sw : w1;
    if (s0 >= s1) return;  // (no workgroup barrier anywhere in this kernel)
    float *cell = acc + (s0 - w0);
    const int32_t len = (int32_t)(s1 - s0);
    for (int32_t c = lane; c < len; c += 64) cell[c] = 0.f;
    wave_lds_sync();

    const int64_t hb = ref_ptr[q], he = ref_ptr[q + 1];
    int64_t m = 0;  // known reference items, repeats counted
    int32_t it = -1;
    int64_t b = 0, e = 0;
    if (hb < he) {
        it = ref_items[hb];
        if (it >= 0 && it < n_items) {
            b = s_ptr[it];
            e = s_ptr[it + 1];
        }
    }
    for (int64_t h = hb; h < he; ++h) {
        const bool known = it >= 0 && it < n_items;
        const int64_t cb = b, ce = e;
        if (h + 1 < he) {  // the next row's bounds travel while this one is walked
            it = ref_items[h + 1];
            b = e = 0;
            if (it >= 0 && it < n_items) {
                b = s_ptr[it];
                e = s_ptr[it + 1];
            }
        }
        if (!known) continue;  // unknown item: dropped (association.py:141-142)
        ++m;
        // the row's entries inside the slice: [p0, p1).  The loads of the next four instructions
        // are issued before the cells of the current four are touched (the cells of one row
        // are distinct, so nothing in a row depends on anything else in it)
        int64_t p0, p1;
        wave_bounds(s_idx, cb, ce, (int32_t)s0, (int32_t)s1, p0, p1);
        int32_t c[4], cn[4];
        float v[4], vn[4];
        auto fetch = [&](int64_t k0, int32_t *fc, float *fv) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = k0 + 64 * j;
                fc[j] = k < p1 ? s_idx[k] - (int32_t)s0 : -1;
                fv[j] = k < p1 ? s_val[k] : 0.f;
            }
        };
        fetch(p0 + lane, c, v);
        for (int64_t k0 = p0; k0 < p1; k0 += 4 * 64) {
            fetch(k0 + 4 * 64 + lane, cn, vn);  // (past p1: no load, nothing to add)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c[j] >= 0 && c[j] < len) {
                    const float a = cell[c[j]];
                    cell[c[j]] = MAX ? fmaxf(a, v[j]) : a + v[j];
                }
                c[j] = cn[j];
                v[j] = vn[j];
            }
        }
        wave_lds_sync();  // the next row may name the same cells from other lanes
    }

    const float nan = __builtin_nanf("");
    if ((mark & 1) && m > 0) {  // the query's own items are no candidates
        for (int64_t h = hb + lane; h < he; h += 64) {
            const int64_t own = ref_items[h];
            if (own >= s0 && own < s1) cell[own - s0] = nan;
        }
        wave_lds_sync();
    }
    float *row = out + q * ld_out + s0;
    if (m == 0) {  // no known reference item: nothing to score with (association.py:144-146)
        const float fill = (mark & 2) ? nan : 0.f;
        for (int32_t c = lane; c < len; c += 64) row[c] = fill;
        return;
    }
    const double dm = (double)m;
    for (int32_t c = lane; c < len; c += 64) {
        const float v = cell[c];
        row[c] = MAX ? v : (float)((double)v / dm);
    }
}

}  // namespace lk

extern "C" int32_t lk_assoc_window(void) { return lk::ASSOC_WINDOW; }

extern "C" int lk_assoc_scale(const int64_t *d_indptr, const int32_t *d_indices, float *d_values,
                              const int32_t *d_item_counts, int64_t n_items, int64_t n_groups,
                              int method, double damping, void *stream)
{
    LK_REQUIRE(n_items >= 0 && n_groups >= 0, "lk_assoc_scale: bad shape");
    LK_REQUIRE(method == LK_ASSOC_PROBABILITY || method == LK_ASSOC_LIFT,
               "lk_assoc_scale: unknown method %d", method);
    LK_REQUIRE(damping >= 0.0, "lk_assoc_scale: damping must not be negative");
    if (n_items == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_item_counts, "lk_assoc_scale: null pointer");
    const int64_t grid = n_items < (1 << 20) ? n_items : (1 << 20);
    hipLaunchKernelGGL(lk::assoc_scale_kernel, dim3((unsigned)grid), dim3(256), 0,
                       lk::as_stream(stream), d_indptr, d_indices, d_values, d_item_counts,
                       n_items, (float)n_groups, method == LK_ASSOC_LIFT ? 1 : 0, damping);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_assoc_score_batch(const int64_t *d_ref_ptr, const int32_t *d_ref_items,
                                    int64_t n_queries, const int64_t *d_s_indptr,
                                    const int32_t *d_s_indices, const float *d_s_values,
                                    int64_t n_items, int reduce, float *d_out, int64_t ld_out,
                                    int mark_history, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_queries >= 0 && n_items >= 0 && ld_out >= n_items &&
                   n_items < ((int64_t)1 << 31) - 64,
               "lk_assoc_score_batch: bad shape");
    LK_REQUIRE(reduce == LK_ASSOC_MEAN || reduce == LK_ASSOC_MAX,
               "lk_assoc_score_batch: unknown reduction %d", reduce);
    if (n_queries == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_ref_ptr && d_s_indptr && d_out, "lk_assoc_score_batch: null pointer");
    // equally wide windows, whole instructions each, none wider than the LDS accumulator
    const int64_t n_win = (n_items + ASSOC_WINDOW - 1) / ASSOC_WINDOW;
    const int64_t win_w = ((n_items + n_win - 1) / n_win + 63) & ~(int64_t)63;
    LK_REQUIRE(n_queries * n_win < ((int64_t)1 << 31),
               "lk_assoc_score_batch: too many tasks for one call, cut the batch");
    const dim3 grid((unsigned)(n_queries * n_win));
    if (reduce == LK_ASSOC_MAX)
        hipLaunchKernelGGL(assoc_score_kernel<true>, grid, dim3(ASSOC_THREADS), 0,
                           as_stream(stream), d_ref_ptr, d_ref_items, d_s_indptr, d_s_indices,
                           d_s_values, n_items, (int32_t)n_win, (int32_t)win_w, d_out, ld_out,
                           mark_history);
    else
        hipLaunchKernelGGL(assoc_score_kernel<false>, grid, dim3(ASSOC_THREADS), 0,
                           as_stream(stream), d_ref_ptr, d_ref_items, d_s_indptr, d_s_indices,
                           d_s_values, n_items, (int32_t)n_win, (int32_t)win_w, d_out, ld_out,
                           mark_history);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
