// mf_pairs.hip -- ragged (user, item) pair scoring for factor models on gfx950: "these 30 items
// for this user, those 12 for that one", the inference path of a rating predictor
// (`FlexMFScorerBase.__call__`, src/lenskit/flexmf/_base.py:116-164, for many queries at once)
// without forming a row of scores per user.
//
// Layout.  The targets of all queries form one flat array; a wave owns TPW consecutive positions
// of it, whichever queries they belong to, so a long list is split over waves and a batch of
// short lists fills the device all the same.  The wave finds the query of its first position by
// a 64-ary search of the offsets (every lane probes one candidate: log64(n) dependent loads) and
// walks the queries it covers.  For each it loads the user's row ONCE (every sub-wave group asks
// for the same addresses in the same instruction: one fetch) and then scores the query's targets
// `64 / G` at a time: a group of G lanes per target, lane j holding the float4 chunks j, j + G,
// ... of the row -- 16 B per lane, a group reads 16 G contiguous bytes of the item's row.  G is
// the largest power of two not above the row's ceil(k / 4) chunks (at most 64), so the two or
// three bias columns behind a power-of-two embedding cost a second, mostly idle load instead of
// doubling the group.
//
// Arithmetic.  A lane accumulates its chunks in ascending order with fused multiply-adds, then the
// G partial sums are added by an xor butterfly (every lane ends with the same bits).  The order is
// a function of k alone: a score does not depend on its position, its query's other targets or
// the rest of the batch.  No atomics.
//
// Traffic per score: the item's row (4 k bytes, in 64-B sectors), 4 B of item number and 4 B of
// output; the user's row and the offsets are amortised over the targets of a (wave, query).
#include "common.h"

namespace lk {
namespace mfp {

constexpr int WPB = 4;        // waves per workgroup
constexpr int ROUNDS = 16;    // target rounds per wave: TPW = ROUNDS * (64 / G)

// the query q with ptr[q] <= pos < ptr[q + 1] (ptr[0] = 0 <= pos < ptr[n]), wave-uniform
__device__ __forceinline__ int64_t find_query(const int64_t *__restrict__ ptr, int64_t n,
                                              int64_t pos, int lane)
{
    int64_t lo = 0, hi = n;  // ptr[lo] <= pos < ptr[hi]
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t idx = lo + (int64_t)(lane + 1) * step;
        const bool le = idx < hi && ptr[idx] <= pos;  // true for the first few lanes only
        const int cnt = __popcll(__ballot(le));
        lo += cnt * step;
        if (lo + step < hi) hi = lo + step;
    }
    return lo;
}

template <int NCH>
__global__ __launch_bounds__(64 * WPB) void mf_score_pairs_kernel(
    const float *__restrict__ U, int ld_u, int64_t n_users, const float *__restrict__ Q, int ld_q,
    int64_t n_items, int k, int G, const int32_t *__restrict__ user_rows, int64_t n_queries,
    const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items, int64_t total,
    float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int groups = 64 / G;
    const int sub = lane / G, j = lane % G;
    const int64_t tpw = (int64_t)ROUNDS * groups;
    const int64_t pos0 = ((int64_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * tpw;
    if (pos0 >= total) return;
    const int64_t pos1 = pos0 + tpw < total ? pos0 + tpw : total;
    const int chunks = (k + 3) / 4;
    const float nan = __builtin_nanf("");

    int64_t q = find_query(tgt_ptr, n_queries, pos0, lane);
    int64_t p = pos0;
    while (p < pos1 && q < n_queries) {
        const int64_t q_end = tgt_ptr[q + 1];
        if (q_end <= p) {  // an empty list (or offsets that do not ascend: nothing is written)
            ++q;
            continue;
        }
        const int64_t end = q_end < pos1 ? q_end : pos1;
        const int32_t urow = user_rows[q];
        const bool user_ok = urow >= 0 && urow < n_users;
        f32x4 u[NCH];
#pragma unroll
        for (int r = 0; r < NCH; ++r) {
            const int c = j + r * G;
            u[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (user_ok && c < chunks)
                u[r] = *reinterpret_cast<const f32x4 *>(U + (int64_t)urow * ld_u + 4 * c);
        }
        for (int64_t t = p + sub; t < end; t += groups) {
            const int32_t item = tgt_items[t];
            const bool ok = user_ok && item >= 0 && item < n_items;
            float acc = 0.0f;
            if (ok) {
#pragma unroll
                for (int r = 0; r < NCH; ++r) {
                    const int c = j + r * G;
                    if (c < chunks) {
                        const f32x4 v =
                            *reinterpret_cast<const f32x4 *>(Q + (int64_t)item * ld_q + 4 * c);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (4 * c + e < k) acc = fmaf(u[r][e], v[e], acc);
                    }
                }
            }
            // the lanes of a group are active together: the butterfly stays inside the group
            for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (j == 0) out[t] = ok ? acc : nan;
        }
        p = end;
        ++q;
    }
}

}  // namespace mfp
}  // namespace lk

extern "C" int lk_mf_score_pairs(const float *d_users, int32_t ld_users, int64_t n_users,
                                 const float *d_items, int32_t ld_items, int64_t n_items,
                                 int32_t k, const int32_t *d_user_rows, int64_t n_queries,
                                 const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                                 int64_t total, float *d_out, void *stream)
{
    LK_REQUIRE(k >= 1 && k <= 1024, "lk_mf_score_pairs: inner width %d outside 1..1024", k);
    const int padded = (k + 3) / 4 * 4;  // whole float4 chunks are read
    LK_REQUIRE(ld_users >= padded && ld_items >= padded && ld_users % 4 == 0 && ld_items % 4 == 0,
               "lk_mf_score_pairs: leading dimensions (%d, %d) must be multiples of 4 and cover "
               "%d columns", ld_users, ld_items, padded);
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_queries >= 0 && total >= 0,
               "lk_mf_score_pairs: bad shape");
    if (total == 0) return LK_OK;
    LK_REQUIRE(n_queries >= 1, "lk_mf_score_pairs: targets without a query");
    LK_REQUIRE(d_users && d_items && d_user_rows && d_tgt_ptr && d_tgt_items && d_out,
               "lk_mf_score_pairs: null pointer");
    LK_REQUIRE(((uintptr_t)d_users | (uintptr_t)d_items) % 16 == 0,
               "lk_mf_score_pairs: operand matrices must be 16-byte aligned");
    const int chunks = (k + 3) / 4;
    int G = 1;
    while (G < 64 && 2 * G <= chunks) G *= 2;
    const int nch = (chunks + G - 1) / G;  // <= 2 below 64 lanes, <= 4 at k <= 1024
    const int64_t tpw = (int64_t)lk::mfp::ROUNDS * (64 / G);
    const int64_t waves = (total + tpw - 1) / tpw;
    const int64_t blocks = (waves + lk::mfp::WPB - 1) / lk::mfp::WPB;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_mf_score_pairs: too many targets");
    const dim3 grid((unsigned)blocks), blk(64 * lk::mfp::WPB);
    hipStream_t st = lk::as_stream(stream);
#define LK_MFP(NCH)                                                                              \
    hipLaunchKernelGGL((lk::mfp::mf_score_pairs_kernel<NCH>), grid, blk, 0, st, d_users,         \
                       (int)ld_users, n_users, d_items, (int)ld_items, n_items, (int)k, G,       \
                       d_user_rows, n_queries, d_tgt_ptr, d_tgt_items, total, d_out)
    if (nch == 1) LK_MFP(1);
    else if (nch == 2) LK_MFP(2);
    else if (nch == 3) LK_MFP(3);
    else LK_MFP(4);
#undef LK_MFP
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
