// stochastic.hip -- the key panel of the stochastic top-N ranker (exponential-sort sampling of a
// Plackett-Luce ranking, src/lenskit/stochastic/_ranker.py:119-156) for whole batches of score
// rows.  A plain top-N of a key row (lk_argtopn) is one sampled ranking.
//
//   key      g = log w~ - log(-log u),  log w~ = max(log w, log FLT_MIN)
//            The reference's key is log(u) / max(w, tiny) = -exp(-g): the same order, but in
//            float32 it overflows to -inf once w sits on the clamp; g is finite for every valid
//            entry (|g| < 105).
//   w        softmax: log w = x - max - log sum exp(x - max);  linear: w = t / sum t with
//            t = (x - min) / (max - min), 1/N when max == min or the sum is 0;  none: w = x.
//            x = score * scale; only finite scores outside the row's exclusion list take part.
//   u        Philox4x32-10, key = seed, counter = (item >> 2, sample, stream lo, stream hi), word
//            item & 3 = b:  u = (2 (b >> 9) + 1) 2^-24 -- exact in float32, never 0, never 1.  A draw
//            depends on (seed, stream, sample, item number) alone.
//   -log u   OCML logf, and -log1pf(-(1 - u)) above 0.5 where 1 - u is exact: the relative accuracy
//            holds up to u = 1 - 2^-24.
//
// Kernels (no float atomics; every reduction has one order, fixed by the row length alone):
//   stoch_stats_kernel  one workgroup per row: max / min / count, then the sum, from two sweeps
//                       over the row (the second one is served by the L2);
//   stoch_keys_kernel   a thread per aligned group of four items (one Philox call, one float4 load
//                       and store where the row is 16-byte aligned, scalar accesses otherwise and
//                       at the tail);
//   stoch_bits_kernel   the key function on given random words (the tests reach the ends of u).
// An item's membership in the sorted exclusion row is a binary search for the group's first item
// followed by a walk over at most the group's entries.
#include "stochastic_shared.h"

namespace lk {

namespace {

using namespace stoch;

struct Quad {
    float v[4];
};

// items [first, first + 4) of a row: NaN past the end of the row
__device__ __forceinline__ Quad load_quad(const float *__restrict__ row, int64_t first,
                                          int64_t row_len, bool aligned)
{
    Quad q;
    if (aligned && first + 4 <= row_len) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(row + first);
        q.v[0] = x[0], q.v[1] = x[1], q.v[2] = x[2], q.v[3] = x[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = first + j < row_len ? row[first + j] : NAN;
    }
    return q;
}

// bit j: item first + j is in the sorted exclusion row cols[lo, hi)
__device__ __forceinline__ unsigned quad_mask(const int32_t *__restrict__ cols, int64_t lo,
                                              int64_t hi, int64_t first)
{
    if (lo >= hi) return 0u;
    int64_t l = lo, h = hi;
    while (l < h) {  // lower bound of `first`
        const int64_t mid = l + ((h - l) >> 1);
        if (cols[mid] < first) l = mid + 1;
        else h = mid;
    }
    unsigned mask = 0u;
    for (; l < hi; ++l) {  // (a repeated entry sets its bit again)
        const int64_t d = (int64_t)cols[l] - first;
        if (d >= 4) break;
        mask |= 1u << (unsigned)d;
    }
    return mask;
}

__device__ __forceinline__ bool takes_part(float score, unsigned mask, int j)
{
    return isfinite(score) && !((mask >> j) & 1u);
}

// stats row: max, min, sum (float), count (int32 bits)
template <int BLK>
__global__ __launch_bounds__(BLK) void stoch_stats_kernel(
    const float *__restrict__ panel, int64_t ld, int64_t row_len,
    const int64_t *__restrict__ excl_ptr, const int32_t *__restrict__ excl_items, int transform,
    float scale, float *__restrict__ stats)
{
    __shared__ float lds[BLK / WAVE];
    const int64_t r = blockIdx.x;
    const float *row = panel + r * ld;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    const int64_t elo = excl_ptr ? excl_ptr[r] : 0, ehi = excl_ptr ? excl_ptr[r + 1] : 0;
    const int64_t nq = (row_len + 3) >> 2;

    float mx = -INFINITY, mn = INFINITY, cnt = 0.f;
    for (int64_t q = threadIdx.x; q < nq; q += BLK) {
        const Quad s = load_quad(row, q * 4, row_len, aligned);
        const unsigned mask = quad_mask(excl_items, elo, ehi, q * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (takes_part(s.v[j], mask, j)) {
                const float x = s.v[j] * scale;
                mx = fmaxf(mx, x);
                mn = fminf(mn, x);
                cnt += 1.f;  // (a thread sees far fewer than 2^24 items: exact)
            }
        }
    }
    mx = block_reduce<BLK>(mx, lds, OpMax());
    mn = block_reduce<BLK>(mn, lds, OpMin());
    // the count as a sum of exact small integers: per thread < 2^24, and the partial sums of a row
    // shorter than 2^24 items stay exact; longer rows are counted in two halves of the bits
    const int my = (int)cnt;
    const float lo16 = block_reduce<BLK>((float)(my & 0xffff), lds, OpAdd());
    const float hi16 = block_reduce<BLK>((float)(my >> 16), lds, OpAdd());
    const int64_t n = (int64_t)lo16 + ((int64_t)hi16 << 16);

    float sum = 0.f;
    const float range = mx - mn;
    if (has_sum(transform, range)) {
        for (int64_t q = threadIdx.x; q < nq; q += BLK) {
            const Quad s = load_quad(row, q * 4, row_len, aligned);
            const unsigned mask = quad_mask(excl_items, elo, ehi, q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (takes_part(s.v[j], mask, j)) {
                    sum += sum_term(s.v[j], scale, mx, mn, range, transform);
                }
            }
        }
        sum = block_reduce<BLK>(sum, lds, OpAdd());
    }
    if (threadIdx.x == 0) {
        float *out = stats + r * 4;
        out[0] = mx;
        out[1] = mn;
        out[2] = sum;
        out[3] = __builtin_bit_cast(float, (int32_t)n);
    }
}

__global__ __launch_bounds__(256) void stoch_keys_kernel(
    const float *__restrict__ panel, int64_t ld, int64_t row_len, int64_t blocks_per_row,
    const int64_t *__restrict__ excl_ptr, const int32_t *__restrict__ excl_items, int transform,
    float scale, const float *__restrict__ stats, uint32_t seed_lo, uint32_t seed_hi,
    const uint64_t *__restrict__ streams, uint32_t sample, float *__restrict__ keys, int64_t ld_keys)
{
    const int64_t r = blockIdx.x / blocks_per_row;
    const int64_t q = (blockIdx.x % blocks_per_row) * 256 + threadIdx.x;
    const int64_t first = q * 4;
    if (first >= row_len) return;
    const float *row = panel + r * ld;
    float *out = keys + r * ld_keys;
    const Quad s = load_quad(row, first, row_len, (reinterpret_cast<uintptr_t>(row) & 15u) == 0);
    const int64_t elo = excl_ptr ? excl_ptr[r] : 0, ehi = excl_ptr ? excl_ptr[r + 1] : 0;
    const unsigned mask = quad_mask(excl_items, elo, ehi, first);

    const float mx = stats[r * 4], mn = stats[r * 4 + 1], sum = stats[r * 4 + 2];
    const int32_t n = __builtin_bit_cast(int32_t, stats[r * 4 + 3]);
    const float range = mx - mn;
    const bool uniform = uniform_weights(range, sum);
    const float log_sum = transform == LK_STOCHASTIC_SOFTMAX ? logf(sum) : 0.f;
    const float log_unif = -logf((float)n);

    const uint64_t stream = streams[r];
    uint32_t c[4] = {(uint32_t)q, sample, (uint32_t)stream, (uint32_t)(stream >> 32)};
    Philox{seed_lo, seed_hi}(c);

    Quad g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float logw = log_weight(s.v[j], scale, mx, mn, range, sum, uniform, log_sum,
                                      log_unif, transform);
        g.v[j] = takes_part(s.v[j], mask, j) ? key_of(logw, c[j]) : NAN;
    }
    if (first + 4 <= row_len && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
        f32x4 o = {g.v[0], g.v[1], g.v[2], g.v[3]};
        *reinterpret_cast<f32x4 *>(out + first) = o;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (first + j < row_len) out[first + j] = g.v[j];
    }
}

__global__ __launch_bounds__(256) void stoch_bits_kernel(const float *__restrict__ logw,
                                                         const uint32_t *__restrict__ bits,
                                                         int64_t n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = key_of(logw[i], bits[i]);
}

}  // namespace

}  // namespace lk

extern "C" int lk_stochastic_row_stats(const float *d_scores, int64_t n_rows, int64_t row_len,
                                       int64_t ld, const int64_t *d_excl_ptr,
                                       const int32_t *d_excl_items, int32_t transform, float scale,
                                       float *d_stats, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_rows >= 0 && row_len >= 0 && ld >= row_len && n_rows < ((int64_t)1 << 31) &&
                   row_len < ((int64_t)1 << 31) - 4,
               "lk_stochastic_row_stats: bad shape");
    LK_REQUIRE(!bad_transform(transform), "lk_stochastic_row_stats: unknown transform %d",
               transform);
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_stats && (row_len == 0 || d_scores), "lk_stochastic_row_stats: null pointer");
    // a wave for short rows, a workgroup for long ones: chosen by the row length alone, so a row
    // reduces in the same order in every batch
    if (row_len <= STATS_WAVE_MAX)
        hipLaunchKernelGGL(stoch_stats_kernel<64>, dim3((unsigned)n_rows), dim3(64), 0,
                           as_stream(stream), d_scores, ld, row_len, d_excl_ptr, d_excl_items,
                           transform, scale, d_stats);
    else
        hipLaunchKernelGGL(stoch_stats_kernel<256>, dim3((unsigned)n_rows), dim3(256), 0,
                           as_stream(stream), d_scores, ld, row_len, d_excl_ptr, d_excl_items,
                           transform, scale, d_stats);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_stochastic_keys(const float *d_scores, int64_t n_rows, int64_t row_len,
                                  int64_t ld, const int64_t *d_excl_ptr,
                                  const int32_t *d_excl_items, int32_t transform, float scale,
                                  const float *d_stats, uint64_t seed, const uint64_t *d_streams,
                                  uint32_t sample, float *d_keys, int64_t ld_keys, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_rows >= 0 && row_len >= 0 && ld >= row_len && ld_keys >= row_len &&
                   row_len < ((int64_t)1 << 31) - 4,
               "lk_stochastic_keys: bad shape");
    LK_REQUIRE(!bad_transform(transform), "lk_stochastic_keys: unknown transform %d", transform);
    if (n_rows == 0 || row_len == 0) return LK_OK;
    LK_REQUIRE(d_scores && d_stats && d_streams && d_keys, "lk_stochastic_keys: null pointer");
    const int64_t blocks_per_row = (((row_len + 3) >> 2) + 255) / 256;
    LK_REQUIRE(n_rows * blocks_per_row < ((int64_t)1 << 31),
               "lk_stochastic_keys: %lld rows of %lld items exceed one launch; split the rows",
               (long long)n_rows, (long long)row_len);
    hipLaunchKernelGGL(stoch_keys_kernel, dim3((unsigned)(n_rows * blocks_per_row)), dim3(256), 0,
                       as_stream(stream), d_scores, ld, row_len, blocks_per_row, d_excl_ptr,
                       d_excl_items, transform, scale, d_stats, (uint32_t)seed,
                       (uint32_t)(seed >> 32), d_streams, sample, d_keys, ld_keys);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_stochastic_key_of_bits(const float *d_log_weight, const uint32_t *d_bits,
                                         int64_t n, float *d_out, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 39), "lk_stochastic_key_of_bits: bad length");
    if (n == 0) return LK_OK;
    LK_REQUIRE(d_log_weight && d_bits && d_out, "lk_stochastic_key_of_bits: null pointer");
    hipLaunchKernelGGL(stoch_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       as_stream(stream), d_log_weight, d_bits, n, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
