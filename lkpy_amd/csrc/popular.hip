// popular.hip -- top-N lists that all come from ONE order (a Popular pipeline's batch path):
// every row's list is the shared, globally sorted item order with that row's own history items
// skipped.  No score panel and no selection: one walk over the order with a membership test.
//
//   rule     row b's list = the first n entries of `order` that do not occur in row b's history,
//            in order; positions past the end are -1 / NaN.  A row without a history (row number
//            -1 or out of range, or no history CSR at all) gets the plain first n.
//   kernel   one wave per row, four waves per workgroup, no LDS, no atomics, no floating-point
//            arithmetic (the scores travel as their 32 bits).  Per step the 64 lanes read the
//            next 64 entries of the order, each lane binary-searches its item in the row's
//            sorted history (repeated entries do not matter to a search), the wave takes a ballot
//            of the kept lanes and each kept lane writes at `emitted + kept lanes below it`.
//            `emitted` is a function of ballots alone, so the loop condition is the same in
//            every lane and no lane leaves before the tail fill.  At most
//            ceil((n + distinct history) / 64) steps.
#include "common.h"

namespace lk {
namespace {

constexpr int SO_WAVES = 4;  // rows per workgroup
constexpr uint32_t SO_NAN_BITS = 0x7fc00000u;

template <typename IT>
__global__ __launch_bounds__(SO_WAVES *WAVE) void shared_order_topn_kernel(
    const int32_t *__restrict__ order, const uint32_t *__restrict__ order_bits, int64_t n_order,
    const IT *__restrict__ hist_ptr, const int32_t *__restrict__ hist_idx, int64_t n_hist_rows,
    const int32_t *__restrict__ rows, int64_t n_rows, int64_t width,
    int32_t *__restrict__ out_idx, uint32_t *__restrict__ out_bits)
{
    const int lane = lane_id();
    const int64_t b = (int64_t)blockIdx.x * SO_WAVES + (threadIdx.x >> 6);
    if (b >= n_rows) return;  // (a whole wave: the kernel has no barrier)
    const int64_t r = rows ? (int64_t)rows[b] : b;
    int64_t lo = 0, hi = 0;
    if (hist_ptr && r >= 0 && r < n_hist_rows) {
        lo = (int64_t)hist_ptr[r];
        hi = (int64_t)hist_ptr[r + 1];
    }
    int32_t *oi = out_idx + b * width;
    uint32_t *ob = out_bits + b * width;

    int64_t emitted = 0;
    for (int64_t base = 0; base < n_order && emitted < width; base += WAVE) {
        const int64_t p = base + lane;
        int32_t item = -1;
        uint32_t bits = SO_NAN_BITS;
        bool keep = false;
        if (p < n_order) {
            item = order[p];
            bits = order_bits[p];
            // lower bound of `item` in the row, then one compare
            int64_t l = lo, h = hi;
            while (l < h) {
                const int64_t mid = l + ((h - l) >> 1);
                if (hist_idx[mid] < item) l = mid + 1;
                else h = mid;
            }
            keep = !(l < hi && hist_idx[l] == item);
        }
        const uint64_t kept = __ballot(keep);
        const unsigned below = __builtin_amdgcn_mbcnt_hi(
            (unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
        const int64_t slot = emitted + below;
        if (keep && slot < width) {
            oi[slot] = item;
            ob[slot] = bits;
        }
        emitted += __popcll(kept);
    }
    if (emitted > width) emitted = width;
    for (int64_t j = emitted + lane; j < width; j += WAVE) {
        oi[j] = -1;
        ob[j] = SO_NAN_BITS;
    }
}

}  // namespace
}  // namespace lk

extern "C" int lk_shared_order_topn(const int32_t *d_order, const float *d_order_scores,
                                    int64_t n_order, const void *d_hist_ptr, int hist_ptr_is_64,
                                    const int32_t *d_hist_idx, int64_t n_hist_rows,
                                    const int32_t *d_rows, int64_t n_rows, int64_t n,
                                    int32_t *d_out_idx, float *d_out_scores, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_order >= 0 && n_hist_rows >= 0 && n_rows >= 0,
               "lk_shared_order_topn: negative size");
    const int64_t width = n < 0 ? n_order : n;
    if (n_rows == 0 || width == 0) return LK_OK;
    LK_REQUIRE(d_out_idx && d_out_scores && (n_order == 0 || (d_order && d_order_scores)),
               "lk_shared_order_topn: null pointer");
    LK_REQUIRE(!d_hist_ptr || d_hist_idx || n_hist_rows == 0,
               "lk_shared_order_topn: offsets without items");
    LK_REQUIRE(d_rows || !d_hist_ptr || n_hist_rows >= n_rows,
               "lk_shared_order_topn: without row numbers the history needs a row per list");
    const int64_t blocks = (n_rows + SO_WAVES - 1) / SO_WAVES;
    LK_REQUIRE(blocks <= (int64_t)INT32_MAX, "lk_shared_order_topn: too many rows");
    const dim3 grid((unsigned)blocks), block(SO_WAVES * WAVE);
    hipStream_t st = as_stream(stream);
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(d_order_scores);
    uint32_t *out_bits = reinterpret_cast<uint32_t *>(d_out_scores);
    if (hist_ptr_is_64)
        hipLaunchKernelGGL(shared_order_topn_kernel<int64_t>, grid, block, 0, st, d_order, bits,
                           n_order, static_cast<const int64_t *>(d_hist_ptr), d_hist_idx,
                           n_hist_rows, d_rows, n_rows, width, d_out_idx, out_bits);
    else
        hipLaunchKernelGGL(shared_order_topn_kernel<int32_t>, grid, block, 0, st, d_order, bits,
                           n_order, static_cast<const int32_t *>(d_hist_ptr), d_hist_idx,
                           n_hist_rows, d_rows, n_rows, width, d_out_idx, out_bits);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
