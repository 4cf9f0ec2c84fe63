// fair.hip -- FA*IR top-N reranking (Zehlike et al. 2017; src/lenskit/reranking/fair.py:198-248) for
// whole batches of ranked lists: one wave per list, no float arithmetic, scores copied as bits.
//
// The reference walks two queues, P (the positions of the protected items, in list order) and U
// (the others), with c the protected count so far; slot i takes
//     P  when  c < m[i] and P is not empty,
//     else the queue whose head position is smaller, else whichever queue is not empty.
// With N[i] = the number of protected items among list positions 0..i, "P's head lies before U's"
// is P[c] <= i, which is N[i] > c (P[c] has P[c] - c unprotected items before it, and U's head
// is unprotected item number i - c).  So slot i takes P exactly when
//     c < h[i],   h[i] = min(|P|, max(m[i], N[i], i + 1 - |U|))
// (the last term: U has run dry), and c' = c + [c < h[i]].  h does not depend on c: it is computed
// a lane per slot, and what remains of the recurrence is a compare and an add per slot on values
// every lane shares, which the compiler keeps in scalar registers.  The slot's source is P[c] or
// U[i - c], read a lane per slot once c is known.
//
// fair_kernel, a wave per row, ROWS waves per workgroup, 12 n_out bytes of LDS per wave
// (P, U and N, n_out entries each):
//   scan    the row in chunks of 64 entries: the flag of every entry from the table (an item
//           number outside it is unprotected), __ballot of the two classes, popcount prefixes;
//           append positions to P and U (the first n_out of each) and N for the first n_out
//           positions.  Without `lengths` the row ends at its first negative entry.  The scan
//           stops at the row's end or once both queues hold n_out positions -- no slot can reach
//           past those.
//   merge   chunks of 64 slots: h a lane per slot, 64 unrolled steps of the recurrence over
//           __builtin_amdgcn_readlane(h, k) collecting a 64-bit mask of the slots that took P, then
//           a lane per slot: c from the mask's popcount prefix, the position from P or U, the item
//           and score gathered from the row, the three outputs written coalesced.
// Every loop is bounded by row_len or n_out.
#include "common.h"

namespace lk {

namespace {

constexpr int FAIR_ROWS = 4;  // waves (rows) per workgroup

__device__ __forceinline__ int popc_below(unsigned long long mask, int lane)
{
    return __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(FAIR_ROWS *WAVE) void fair_kernel(
    const int32_t *__restrict__ lists, int64_t n_rows, int32_t row_len, int64_t ld,
    const int32_t *__restrict__ lengths, const uint32_t *__restrict__ scores,
    const uint8_t *__restrict__ is_protected, int64_t n_items, const int32_t *__restrict__ m_table,
    int32_t n_out, int32_t *__restrict__ out_items, uint32_t *__restrict__ out_scores,
    int32_t *__restrict__ out_pos)
{
    extern __shared__ int32_t fair_lds[];
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * FAIR_ROWS + w;
    if (r >= n_rows) return;  // (whole waves; the kernel has no workgroup barrier)
    int32_t *qp = fair_lds + (size_t)w * 3 * n_out;
    int32_t *qu = qp + n_out;
    int32_t *cum = qu + n_out;
    const int32_t *row = lists + r * ld;

    // ---- scan ------------------------------------------------------------------------------
    int len = row_len;
    if (lengths) len = min(max(lengths[r], 0), row_len);
    int np = 0, nu = 0;  // protected / unprotected entries seen (wave-uniform)
    for (int base = 0; base < len; base += WAVE) {
        const int j = base + lane;
        const int item = j < len ? row[j] : 0;
        if (!lengths) {  // the row ends at its first negative entry
            const unsigned long long neg = __ballot(j < len && item < 0);
            if (neg) len = base + __ffsll((long long)neg) - 1;
        }
        const bool valid = j < len;
        const bool prot = valid && item >= 0 && (int64_t)item < n_items && is_protected[item] != 0;
        const unsigned long long pm = __ballot(prot), um = __ballot(valid && !prot);
        const int pi = np + popc_below(pm, lane), ui = nu + popc_below(um, lane);
        if (prot && pi < n_out) qp[pi] = j;
        if (valid && !prot && ui < n_out) qu[ui] = j;
        if (valid && j < n_out) cum[j] = pi + (prot ? 1 : 0);
        np += __popcll(pm);
        nu += __popcll(um);
        if (np >= n_out && nu >= n_out) break;  // (at least 2 n_out entries seen)
    }
    wave_lds_sync();

    // ---- merge -----------------------------------------------------------------------------
    const int n_eff = min(n_out, len);
    int32_t *o_items = out_items + r * (int64_t)n_out;
    uint32_t *o_scores = out_scores ? out_scores + r * (int64_t)n_out : nullptr;
    int32_t *o_pos = out_pos ? out_pos + r * (int64_t)n_out : nullptr;
    const uint32_t *srow = scores ? scores + r * ld : nullptr;
    int c0 = 0;
    for (int base = 0; base < n_out; base += WAVE) {
        const int i = base + lane;
        int h = 0;
        if (i < n_eff) h = min(np, max(max(m_table[i], cum[i]), i + 1 - nu));
        int c = __builtin_amdgcn_readfirstlane(c0);
        unsigned long long took = 0ull;
        if (base < n_eff) {
#pragma unroll
            for (int k = 0; k < WAVE; ++k) {
                const int t = c < __builtin_amdgcn_readlane(h, k) ? 1 : 0;
                took |= (unsigned long long)t << k;
                c += t;
            }
        }
        if (i < n_out) {
            int pos = -1, item = -1;
            uint32_t sc = 0x7fc00000u;  // NaN
            if (i < n_eff) {
                const int ci = c0 + popc_below(took, lane);
                // (the indices are in range by construction; the clamps keep a wrong table or
                // length from reaching outside the queues and the row)
                const int qi = min(max(((took >> lane) & 1ull) ? ci : i - ci, 0), n_out - 1);
                pos = ((took >> lane) & 1ull) ? qp[qi] : qu[qi];
                pos = min(max(pos, 0), row_len - 1);
                item = row[pos];
                if (srow) sc = srow[pos];
            }
            o_items[i] = item;
            if (o_scores) o_scores[i] = sc;
            if (o_pos) o_pos[i] = pos;
        }
        c0 = c;
    }
}

}  // namespace

}  // namespace lk

extern "C" int32_t lk_fair_max_n(void) { return LK_FAIR_MAX_N; }

extern "C" int lk_fair_rerank(const int32_t *d_lists, int64_t n_rows, int64_t row_len, int64_t ld,
                              const int32_t *d_lengths, const float *d_scores,
                              const uint8_t *d_is_protected, int64_t n_items,
                              const int32_t *d_m_table, int32_t n_table, int32_t n_out,
                              int32_t *d_out_items, float *d_out_scores, int32_t *d_out_pos,
                              void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_rows >= 0 && row_len >= 0 && ld >= row_len && n_items >= 0 &&
                   row_len < ((int64_t)1 << 31) - WAVE &&
                   n_rows < ((int64_t)1 << 31) * FAIR_ROWS - FAIR_ROWS,
               "lk_fair_rerank: bad shape");
    LK_REQUIRE(n_table >= 0 && n_table <= LK_FAIR_MAX_N,
               "lk_fair_rerank: a threshold table of %d entries is over the limit of %d", n_table,
               LK_FAIR_MAX_N);
    LK_REQUIRE(n_out >= 0 && n_out <= n_table,
               "lk_fair_rerank: n_out = %d outside the threshold table's 0..%d", n_out, n_table);
    LK_REQUIRE(!d_out_scores || d_scores, "lk_fair_rerank: null pointer (scores out without in)");
    if (n_rows == 0 || n_out == 0) return LK_OK;
    LK_REQUIRE(d_out_items && d_m_table && (row_len == 0 || d_lists) &&
                   (n_items == 0 || d_is_protected),
               "lk_fair_rerank: null pointer");
    const unsigned blocks = (unsigned)((n_rows + FAIR_ROWS - 1) / FAIR_ROWS);
    const size_t lds = (size_t)FAIR_ROWS * 3 * (size_t)n_out * sizeof(int32_t);
    hipLaunchKernelGGL(fair_kernel, dim3(blocks), dim3(FAIR_ROWS * WAVE), lds, as_stream(stream),
                       d_lists, n_rows, (int32_t)row_len, ld, d_lengths,
                       reinterpret_cast<const uint32_t *>(d_scores), d_is_protected, n_items,
                       d_m_table, n_out, d_out_items, reinterpret_cast<uint32_t *>(d_out_scores),
                       d_out_pos);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
