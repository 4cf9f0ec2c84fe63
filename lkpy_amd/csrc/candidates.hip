// candidates.hip -- per-query candidate lists on gfx950: "score THESE items for this user, rank
// them, keep n" for a whole batch of queries (`BatchRecRequest.candidates`,
// src/lenskit/batch/_queries.py:50-78; `pipe.run("recommender", query=, items=, n=)` and
// `BatchPipelineRunner.score`, src/lenskit/batch/_runner.py:114-124, for many queries at once).
//
// Layout, shared by the three entry points: the targets of all queries form one flat array,
// query q owns the positions [tgt_ptr[q], tgt_ptr[q + 1]) (int64 offsets ascending from 0,
// empty lists allowed anywhere).  A thread that needs the query of a position finds it by a
// binary search of the offsets (log2(n_queries) L2-served loads); every offset it then uses is
// clamped to [0, total], every item number and user row is range-checked before it becomes an
// address.
//
//   lk_score_candidates   the inner products of ragged (user row, item) pairs as the SINGLE
//                         k-ordered fused-multiply-add chain of lk_score_dense (topk.hip: the f32
//                         MFMA is that chain bit for bit), where lk_mf_score_pairs adds per-lane
//                         partial sums.  A wave owns 64 consecutive targets, whichever queries they
//                         belong to; the 64 item rows are loaded coalesced, SLAB columns at a time
//                         (8 lanes x 16 B per row), into an LDS tile of row stride SLAB + 1 floats,
//                         then lane l walks row l in column order (stride 33: conflict-free) and
//                         carries its accumulator from slab to slab.  The user's row is read by
//                         the lane itself, 16 B at a time: the lanes of a query ask for the same
//                         addresses in the same instruction.  Traffic per score: the item's row
//                         (4 k bytes, in 128-B runs), 4 B of item number, 4 B of output.
//   lk_panel_take_ragged  out[t] = panel[q][item[t]]: lk_take_scores for ragged targets.
//   lk_ragged_topn        lk_argtopn per segment: NaN scores and negative items dropped, the rest
//                         by descending f2key order, ties to the lower position.  Every entry gets
//                         the unique 64-bit key (inverted f2key << 32 | position), an invalid one
//                         the inverted key 0xffffffff behind every valid one, so an entry's rank
//                         is the number of smaller keys of its segment and the ranks of a segment
//                         are a permutation of 0 .. len - 1: the entry of rank r writes slot r (its
//                         item and its score's own bits, or the padding if it is invalid), slots
//                         from len on are padded.  Three classes by segment length:
//                           <= WAVE_MAX (64)     one wave, keys in registers, rank by counting
//                                                over lane broadcasts;
//                           <= BLOCK_MAX (1024)  one workgroup, keys in LDS, rank by counting
//                                                (every thread reads the same key: a broadcast);
//                           longer               one stable radix sort (radix_sort.h) of
//                                                (query << 32 | inverted key) over the batch --
//                                                segment q then occupies [ptr[q], ptr[q + 1]) of
//                                                the sorted array -- and an emit pass that writes
//                                                the long segments only.
// No atomics; a result depends on its own segment alone.
#include "common.h"
#include "radix_sort.h"
#include "ragged.h"

namespace lk {
namespace cand {

constexpr int WPB = 4;            // waves per workgroup
constexpr int SLAB = 32;          // item columns staged per pass
constexpr int TLD = SLAB + 1;     // tile row stride: lane l reads bank (l + c) % 32
constexpr int WAVE_MAX = 64;      // longest segment ranked by one wave
constexpr int BLOCK_MAX = 1024;   // longest segment ranked by one workgroup in LDS
constexpr int BLOCK_T = 256;
constexpr int PER_T = BLOCK_MAX / BLOCK_T;

using ragged::clampi;
using ragged::query_of;

__global__ __launch_bounds__(64 * WPB) void score_candidates_kernel(
    const float *__restrict__ U, int ld_u, int64_t n_users, const float *__restrict__ Q, int ld_q,
    int64_t n_items, int k, const int32_t *__restrict__ user_rows, int64_t n_queries,
    const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items, int64_t total,
    float *__restrict__ out)
{
    __shared__ float tiles[WPB][64 * TLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *tile = tiles[wave];
    const int64_t pos0 = ((int64_t)blockIdx.x * WPB + wave) * 64;
    if (pos0 >= total) return;  // (wave-uniform; no workgroup barrier below)
    const int64_t t = pos0 + lane;
    const bool live = t < total;
    int32_t item = -1, urow = -1;
    if (live) {
        item = tgt_items[t];
        urow = user_rows[query_of(tgt_ptr, n_queries, t)];
    }
    const bool item_ok = item >= 0 && item < n_items;
    const bool ok = item_ok && urow >= 0 && urow < n_users;
    if (!item_ok) item = -1;
    const float *urow_p = U + (int64_t)(ok ? urow : 0) * ld_u;
    const int padded = (k + 3) / 4 * 4;
    const int r_sub = lane >> 3, c4 = (lane & 7) * 4;  // this lane's (row in a step, column)
    float acc = 0.0f;
    for (int s0 = 0; s0 < k; s0 += SLAB) {
        // 8 steps of 8 rows: 8 lanes read 128 contiguous bytes of one item's row
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = i * 8 + r_sub;
            const int32_t it = __shfl(item, r, 64);
            f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (it >= 0 && s0 + c4 < padded)
                v = *reinterpret_cast<const f32x4 *>(Q + (int64_t)it * ld_q + s0 + c4);
            float *dst = tile + r * TLD + c4;
            dst[0] = v[0];
            dst[1] = v[1];
            dst[2] = v[2];
            dst[3] = v[3];
        }
        wave_lds_sync();
        const float *row = tile + lane * TLD;
        for (int c = 0; c < SLAB && s0 + c < k; c += 4) {
            f32x4 u = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (ok) u = *reinterpret_cast<const f32x4 *>(urow_p + s0 + c);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s0 + c + e < k) acc = __builtin_fmaf(u[e], row[c + e], acc);
        }
        wave_lds_sync();  // the tile is read before the next slab overwrites it
    }
    if (live) out[t] = ok ? acc : __builtin_nanf("");
}

__global__ __launch_bounds__(256) void panel_take_ragged_kernel(
    const float *__restrict__ panel, int64_t n_rows, int64_t n_items, int64_t ld,
    const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_items, int64_t total,
    float *__restrict__ out)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t item = tgt_items[t];
        float v = __builtin_nanf("");
        if (item >= 0 && item < n_items)
            v = panel[query_of(tgt_ptr, n_rows, t) * ld + item];
        out[t] = v;
    }
}

// ---- ranking ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t inv_key(float score, int32_t item)
{
    // every valid key is >= f2key(-inf) > 0, so a valid inverted key is below 0xffffffff
    return (score == score && item >= 0) ? 0xffffffffu - f2key(score) : 0xffffffffu;
}

__device__ __forceinline__ void put(int32_t *__restrict__ out_idx, float *__restrict__ out_score,
                                    int64_t at, bool valid, int32_t item, float score)
{
    out_idx[at] = valid ? item : -1;
    out_score[at] = valid ? score : __builtin_nanf("");
}

__global__ __launch_bounds__(64 * WPB) void ragged_topn_wave_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ items,
    const float *__restrict__ scores, int64_t total, int64_t width,
    int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (q >= n_queries) return;
    const int64_t lo = clampi(tgt_ptr[q], 0, total), hi = clampi(tgt_ptr[q + 1], lo, total);
    const int len = hi - lo > WAVE_MAX ? -1 : (int)(hi - lo);
    if (len < 0) return;  // (another class: wave-uniform)
    int32_t item = -1;
    float score = __builtin_nanf("");
    if (lane < len) {
        item = items[lo + lane];
        score = scores[lo + lane];
    }
    const uint32_t inv = inv_key(score, item);
    const unsigned long long key = ((unsigned long long)inv << 32) | (unsigned)lane;
    int rank = 0;
    for (int j = 0; j < len; ++j) {
        const unsigned long long other = __shfl(key, j, 64);
        rank += other < key ? 1 : 0;
    }
    if (lane < len && rank < width)
        put(out_idx, out_score, q * width + rank, inv != 0xffffffffu, item, score);
    for (int64_t j = len + lane; j < width; j += 64)
        put(out_idx, out_score, q * width + j, false, -1, 0.0f);
}

__global__ __launch_bounds__(BLOCK_T) void ragged_topn_block_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ items,
    const float *__restrict__ scores, int64_t total, int64_t width,
    int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    __shared__ unsigned long long keys[BLOCK_MAX];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t lo = clampi(tgt_ptr[q], 0, total), hi = clampi(tgt_ptr[q + 1], lo, total);
    if (hi - lo <= WAVE_MAX || hi - lo > BLOCK_MAX) return;  // (another class: uniform)
    const int len = (int)(hi - lo);
    int32_t item[PER_T];
    float score[PER_T];
    unsigned long long key[PER_T];
    int rank[PER_T];
#pragma unroll
    for (int r = 0; r < PER_T; ++r) {
        const int i = tid + r * BLOCK_T;
        item[r] = -1;
        score[r] = __builtin_nanf("");
        key[r] = ~0ull;
        rank[r] = 0;
        if (i < len) {
            item[r] = items[lo + i];
            score[r] = scores[lo + i];
            key[r] = ((unsigned long long)inv_key(score[r], item[r]) << 32) | (unsigned)i;
            keys[i] = key[r];
        }
    }
    __syncthreads();
    for (int j = 0; j < len; ++j) {
        const unsigned long long other = keys[j];
#pragma unroll
        for (int r = 0; r < PER_T; ++r) rank[r] += other < key[r] ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < PER_T; ++r) {
        const int i = tid + r * BLOCK_T;
        if (i < len && rank[r] < width)
            put(out_idx, out_score, q * width + rank[r], (uint32_t)(key[r] >> 32) != 0xffffffffu,
                item[r], score[r]);
    }
    for (int64_t j = len + tid; j < width; j += BLOCK_T)
        put(out_idx, out_score, q * width + j, false, -1, 0.0f);
}

__global__ __launch_bounds__(256) void ragged_sort_keys_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ items,
    const float *__restrict__ scores, int64_t total, unsigned long long *__restrict__ keys,
    uint32_t *__restrict__ vals)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long q = (unsigned long long)query_of(tgt_ptr, n_queries, t);
        keys[t] = (q << 32) | inv_key(scores[t], items[t]);
        vals[t] = (uint32_t)t;
    }
}

// sorted entry e belongs to the query in its key's upper half; that query's entries are
// [ptr[q], ptr[q + 1]) of the sorted array, so e - ptr[q] is the entry's rank
__global__ __launch_bounds__(256) void ragged_sort_emit_kernel(
    int64_t n_queries, const int64_t *__restrict__ tgt_ptr, const int32_t *__restrict__ items,
    const float *__restrict__ scores, int64_t total, const unsigned long long *__restrict__ keys,
    const uint32_t *__restrict__ vals, int64_t width, int32_t *__restrict__ out_idx,
    float *__restrict__ out_score)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[e];
        const int64_t q = (int64_t)(key >> 32);
        if (q >= n_queries) continue;
        const int64_t lo = clampi(tgt_ptr[q], 0, total), hi = clampi(tgt_ptr[q + 1], lo, total);
        const int64_t len = hi - lo, rank = e - lo;
        if (len <= BLOCK_MAX || rank < 0 || rank >= len) continue;
        if (rank < width) {
            const uint32_t t = vals[e];
            const bool valid = (uint32_t)key != 0xffffffffu && t < total;
            put(out_idx, out_score, q * width + rank, valid, valid ? items[t] : -1,
                valid ? scores[t] : 0.0f);
        }
        for (int64_t j = rank + len; j < width; j += len)
            put(out_idx, out_score, q * width + j, false, -1, 0.0f);
    }
}

static int query_bits(int64_t n_queries)
{
    int b = 0;
    while (((int64_t)1 << b) < n_queries) ++b;
    return b;
}

static unsigned stride_grid(int64_t n)
{
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g < 8192 ? g : 8192));
}

}  // namespace cand
}  // namespace lk

extern "C" int lk_score_candidates(const float *d_users, int32_t ld_users, int64_t n_users,
                                   const float *d_items, int32_t ld_items, int64_t n_items,
                                   int32_t k, const int32_t *d_user_rows, int64_t n_queries,
                                   const int64_t *d_tgt_ptr, const int32_t *d_tgt_items,
                                   int64_t total, float *d_out, void *stream)
{
    LK_REQUIRE(k >= 1 && k <= 1024, "lk_score_candidates: inner width %d outside 1..1024", k);
    const int padded = (k + 3) / 4 * 4;  // whole float4 chunks are read
    LK_REQUIRE(ld_users >= padded && ld_items >= padded && ld_users % 4 == 0 && ld_items % 4 == 0,
               "lk_score_candidates: leading dimensions (%d, %d) must be multiples of 4 and cover "
               "%d columns", ld_users, ld_items, padded);
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_queries >= 0 && total >= 0,
               "lk_score_candidates: bad shape");
    if (total == 0) return LK_OK;
    LK_REQUIRE(n_queries >= 1, "lk_score_candidates: targets without a query");
    LK_REQUIRE(d_users && d_items && d_user_rows && d_tgt_ptr && d_tgt_items && d_out,
               "lk_score_candidates: null pointer");
    LK_REQUIRE(((uintptr_t)d_users | (uintptr_t)d_items) % 16 == 0,
               "lk_score_candidates: operand matrices must be 16-byte aligned");
    const int64_t per_block = 64 * lk::cand::WPB;
    const int64_t blocks = (total + per_block - 1) / per_block;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_score_candidates: too many targets");
    hipLaunchKernelGGL(lk::cand::score_candidates_kernel, dim3((unsigned)blocks),
                       dim3(64 * lk::cand::WPB), 0, lk::as_stream(stream), d_users, (int)ld_users,
                       n_users, d_items, (int)ld_items, n_items, (int)k, d_user_rows, n_queries,
                       d_tgt_ptr, d_tgt_items, total, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_panel_take_ragged(const float *d_panel, int64_t n_queries, int64_t n_items,
                                    int64_t ld, const int64_t *d_tgt_ptr,
                                    const int32_t *d_tgt_items, int64_t total, float *d_out,
                                    void *stream)
{
    LK_REQUIRE(n_queries >= 0 && n_items >= 0 && total >= 0 && ld >= n_items,
               "lk_panel_take_ragged: bad shape");
    if (total == 0) return LK_OK;
    LK_REQUIRE(n_queries >= 1, "lk_panel_take_ragged: targets without a query");
    LK_REQUIRE(d_tgt_ptr && d_tgt_items && d_out && (d_panel || n_items == 0),
               "lk_panel_take_ragged: null pointer");
    hipLaunchKernelGGL(lk::cand::panel_take_ragged_kernel, dim3(lk::cand::stride_grid(total)),
                       dim3(256), 0, lk::as_stream(stream), d_panel, n_queries, n_items, ld,
                       d_tgt_ptr, d_tgt_items, total, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int32_t lk_ragged_topn_wave_max(void) { return lk::cand::WAVE_MAX; }

extern "C" int32_t lk_ragged_topn_block_max(void) { return lk::cand::BLOCK_MAX; }

extern "C" size_t lk_ragged_topn_workspace_bytes(int64_t total, int64_t max_len)
{
    if (total <= 0 || max_len <= lk::cand::BLOCK_MAX) return 0;
    const size_t e = (size_t)total;
    // keys in / out / ping-pong (8 B), values in / out / ping-pong (4 B), the sort's histogram
    return 3 * lk::align_up(e * 8, 256) + 3 * lk::align_up(e * 4, 256) +
           lk::align_up(lk::radix_sort_temp_bytes(total), 256) + 256;
}

extern "C" int lk_ragged_topn(int64_t n_queries, const int64_t *d_tgt_ptr,
                              const int32_t *d_tgt_items, const float *d_scores, int64_t total,
                              int32_t n, int64_t max_len, void *d_ws, int32_t *d_out_idx,
                              float *d_out_score, void *stream)
{
    using namespace lk::cand;
    LK_REQUIRE(n_queries >= 0 && total >= 0 && max_len >= 0 && max_len <= total,
               "lk_ragged_topn: bad shape");
    LK_REQUIRE(total < ((int64_t)1 << 31), "lk_ragged_topn: more than 2^31 entries in one call");
    const int64_t width = n < 0 ? max_len : (int64_t)n;
    if (n_queries == 0 || width == 0) return LK_OK;
    LK_REQUIRE(d_tgt_ptr && d_out_idx && d_out_score && (total == 0 || (d_tgt_items && d_scores)),
               "lk_ragged_topn: null pointer");
    hipStream_t st = lk::as_stream(stream);
    const int64_t wave_blocks = (n_queries + WPB - 1) / WPB;
    LK_REQUIRE(wave_blocks < ((int64_t)1 << 31), "lk_ragged_topn: too many queries");
    hipLaunchKernelGGL(ragged_topn_wave_kernel, dim3((unsigned)wave_blocks), dim3(64 * WPB), 0, st,
                       n_queries, d_tgt_ptr, d_tgt_items, d_scores, total, width, d_out_idx,
                       d_out_score);
    if (max_len > WAVE_MAX)
        hipLaunchKernelGGL(ragged_topn_block_kernel, dim3((unsigned)n_queries), dim3(BLOCK_T), 0,
                           st, n_queries, d_tgt_ptr, d_tgt_items, d_scores, total, width,
                           d_out_idx, d_out_score);
    if (max_len > BLOCK_MAX) {
        LK_REQUIRE(d_ws, "lk_ragged_topn: segments above %d entries need the workspace of "
                   "lk_ragged_topn_workspace_bytes", BLOCK_MAX);
        const size_t e = (size_t)total;
        char *p = static_cast<char *>(d_ws);
        auto *k_in = reinterpret_cast<unsigned long long *>(p);
        p += lk::align_up(e * 8, 256);
        auto *k_out = reinterpret_cast<unsigned long long *>(p);
        p += lk::align_up(e * 8, 256);
        auto *k_tmp = reinterpret_cast<unsigned long long *>(p);
        p += lk::align_up(e * 8, 256);
        uint32_t *v_in = reinterpret_cast<uint32_t *>(p);
        p += lk::align_up(e * 4, 256);
        uint32_t *v_out = reinterpret_cast<uint32_t *>(p);
        p += lk::align_up(e * 4, 256);
        uint32_t *v_tmp = reinterpret_cast<uint32_t *>(p);
        p += lk::align_up(e * 4, 256);
        hipLaunchKernelGGL(ragged_sort_keys_kernel, dim3(stride_grid(total)), dim3(256), 0, st,
                           n_queries, d_tgt_ptr, d_tgt_items, d_scores, total, k_in, v_in);
        int rc = lk::radix_sort_pairs<unsigned long long, uint32_t>(
            k_in, v_in, k_out, v_out, k_tmp, v_tmp, total, 0, 32 + query_bits(n_queries), p, st);
        if (rc != LK_OK) return rc;
        hipLaunchKernelGGL(ragged_sort_emit_kernel, dim3(stride_grid(total)), dim3(256), 0, st,
                           n_queries, d_tgt_ptr, d_tgt_items, d_scores, total, k_out, v_out, width,
                           d_out_idx, d_out_score);
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
