// ragged_stochastic.hip -- the keys of the stochastic top-N ranker (stochastic.hip) for ragged
// candidate lists: segment s holds the entries of ONE row of a [1 x width_s] score panel -- score
// scores[t] at column addr[t], NaN everywhere else -- and gets the bits lk_stochastic_row_stats and
// lk_stochastic_keys give that row, without the row ever being formed.
//
// What the same bits take:
//   max, min, count  do not depend on the order of the entries.
//   sum (float32)    does.  The panel kernel runs BLK threads per row (64 for width <= 2048, else
//                    256); thread v adds the terms of the quads v, v + BLK, ... in ascending
//                    column order, a 64-lane xor butterfly follows, then the waves' values are
//                    added in wave order.  Entry t therefore BELONGS to thread (addr[t] >> 2) % BLK,
//                    and with addresses that ascend inside a segment a walk over the segment meets
//                    every thread's entries in that thread's order.
//   draws            word addr & 3 of Philox(seed)(addr >> 2, sample, stream lo, stream hi).
// The weight, the key function, the special cases and the terms are those of
// stochastic_shared.h, the expressions the panel kernels inline.
//
// ragged_keys_kernel: ONE WAVE per segment, four segments per workgroup.  Lane l plays the panel
// kernel's threads l, l + 64, ... (one or four accumulators), so the butterfly is the wave's own
// and the wave-order add is three adds in registers: no LDS reduction, no barrier, no atomics.
//   pass 1   max / min / count, lanes striding the segment;
//   pass 2   the segment in chunks of RS_CHUNK entries: lanes stage (term, owner thread) in LDS
//            (8 bytes per entry, one ds_read_b64 that every lane reads at the same address -- a
//            broadcast), then every lane walks the chunk and adds the terms it owns;
//   pass 3   lanes striding the segment again: one Philox call and one key per entry and sample.
// A segment longer than the chunk is walked chunk by chunk by the same wave (the order is kept
// because the chunks are taken in order).  16 KiB of LDS per workgroup: occupancy is bounded by
// the 32 waves of a CU, not by LDS.
//
// The contract is on the caller -- addresses ascend strictly inside a segment and lie in
// [0, width) -- but no input is used as a memory address: an address only enters arithmetic, the
// offsets are clamped to [0, total].  An entry whose address is outside [0, width) takes no part.
#include "stochastic_shared.h"

namespace lk {

namespace {

using namespace stoch;

constexpr int RS_WAVES = 4;    // segments (waves) per workgroup
constexpr int RS_CHUNK = 512;  // entries staged per wave: RS_WAVES * RS_CHUNK * 8 B = 16 KiB

struct Staged {
    float term;
    int32_t owner;  // the panel thread the entry belongs to; -1: the entry takes no part
};

__device__ __forceinline__ bool takes_part(float score, int32_t a, int32_t width)
{
    return isfinite(score) && a >= 0 && a < width;
}

// the staged chunk's terms added by their owners: lane l is the panel threads l + 64 v, v < VT
template <int VT>
__device__ __forceinline__ void walk_chunk(const Staged *chunk, int m, int lane, float (&acc)[4])
{
    for (int i = 0; i < m; ++i) {
        const Staged e = chunk[i];
#pragma unroll
        for (int v = 0; v < VT; ++v) acc[v] = e.owner == lane + WAVE * v ? acc[v] + e.term : acc[v];
    }
}

__device__ __forceinline__ float butterfly_add(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(RS_WAVES *WAVE) void ragged_keys_kernel(
    int64_t n_segments, const int64_t *__restrict__ ptr, int64_t total,
    const int32_t *__restrict__ addr, const float *__restrict__ scores,
    const int32_t *__restrict__ widths, const uint64_t *__restrict__ streams, int transform,
    float scale, uint32_t seed_lo, uint32_t seed_hi, uint32_t first_sample, int32_t samples,
    float *__restrict__ stats, float *__restrict__ keys)
{
    __shared__ Staged stage[RS_WAVES][RS_CHUNK];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * RS_WAVES + w;
    if (s >= n_segments) return;  // (a whole wave; the kernel has no workgroup barrier)
    int64_t lo = ptr[s], hi = ptr[s + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    const int32_t width = widths[s];
    const bool wide = width > STATS_WAVE_MAX;  // the panel kernel's 256 threads

    // pass 1: max, min, count
    float mx = -INFINITY, mn = INFINITY;
    int32_t n = 0;
    for (int64_t t = lo + lane; t < hi; t += WAVE) {
        const float sc = scores[t];
        if (takes_part(sc, addr[t], width)) {
            const float x = sc * scale;
            mx = fmaxf(mx, x);
            mn = fminf(mn, x);
            n += 1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        n += __shfl_xor(n, off, 64);
    }

    // pass 2: the sum, every panel thread's terms in that thread's order
    float sum = 0.f;
    const float range = mx - mn;
    if (has_sum(transform, range)) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        Staged *chunk = stage[w];
        const int32_t owner_mask = wide ? STATS_BLK_LONG - 1 : WAVE - 1;
        for (int64_t c = lo; c < hi; c += RS_CHUNK) {
            const int m = hi - c < RS_CHUNK ? (int)(hi - c) : RS_CHUNK;
            for (int i = lane; i < m; i += WAVE) {
                const float sc = scores[c + i];
                const int32_t a = addr[c + i];
                Staged e;
                e.term = 0.f, e.owner = -1;
                if (takes_part(sc, a, width)) {
                    e.term = sum_term(sc, scale, mx, mn, range, transform);
                    e.owner = (a >> 2) & owner_mask;
                }
                chunk[i] = e;
            }
            wave_lds_sync();
            if (wide) walk_chunk<4>(chunk, m, lane, acc);
            else walk_chunk<1>(chunk, m, lane, acc);
            wave_lds_sync();  // (the next chunk overwrites what this walk read)
        }
        sum = butterfly_add(acc[0]);
        if (wide) {  // the waves' values in wave order
#pragma unroll
            for (int v = 1; v < 4; ++v) sum = sum + butterfly_add(acc[v]);
        }
    }
    if (lane == 0) {
        float *out = stats + s * 4;
        out[0] = mx;
        out[1] = mn;
        out[2] = sum;
        out[3] = __builtin_bit_cast(float, n);
    }

    // pass 3: the keys of every sample
    const bool uniform = uniform_weights(range, sum);
    const float log_sum = transform == LK_STOCHASTIC_SOFTMAX ? logf(sum) : 0.f;
    const float log_unif = -logf((float)n);
    const uint64_t stream = streams[s];
    for (int64_t t = lo + lane; t < hi; t += WAVE) {
        const float sc = scores[t];
        const int32_t a = addr[t];
        const bool part = takes_part(sc, a, width);
        const float logw = log_weight(sc, scale, mx, mn, range, sum, uniform, log_sum, log_unif,
                                      transform);
        for (int32_t j = 0; j < samples; ++j) {
            uint32_t c[4] = {(uint32_t)(a >> 2), first_sample + (uint32_t)j, (uint32_t)stream,
                             (uint32_t)(stream >> 32)};
            Philox{seed_lo, seed_hi}(c);
            const int word = a & 3;
            const uint32_t bits = word == 0 ? c[0] : word == 1 ? c[1] : word == 2 ? c[2] : c[3];
            keys[(int64_t)j * total + t] = part ? key_of(logw, bits) : NAN;
        }
    }
}

}  // namespace

}  // namespace lk

extern "C" int32_t lk_ragged_stochastic_chunk(void) { return lk::RS_CHUNK; }

extern "C" int lk_ragged_stochastic_keys(int64_t n_segments, const int64_t *d_ptr,
                                         const int32_t *d_addr, const float *d_scores,
                                         int64_t total, const int32_t *d_width,
                                         const uint64_t *d_streams, int32_t transform, float scale,
                                         uint64_t seed, uint32_t first_sample, int32_t samples,
                                         float *d_stats, float *d_keys, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_segments >= 0 && total >= 0 && samples >= 0 && total < ((int64_t)1 << 31),
               "lk_ragged_stochastic_keys: bad shape");
    LK_REQUIRE(!stoch::bad_transform(transform), "lk_ragged_stochastic_keys: unknown transform %d",
               transform);
    if (n_segments == 0) return LK_OK;
    LK_REQUIRE(d_ptr && d_width && d_streams && d_stats, "lk_ragged_stochastic_keys: null pointer");
    LK_REQUIRE(total == 0 || (d_addr && d_scores && (samples == 0 || d_keys)),
               "lk_ragged_stochastic_keys: null pointer");
    const int64_t blocks = (n_segments + RS_WAVES - 1) / RS_WAVES;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_ragged_stochastic_keys: too many segments");
    hipLaunchKernelGGL(ragged_keys_kernel, dim3((unsigned)blocks), dim3(RS_WAVES * WAVE), 0,
                       as_stream(stream), n_segments, d_ptr, total, d_addr, d_scores, d_width,
                       d_streams, transform, scale, (uint32_t)seed, (uint32_t)(seed >> 32),
                       first_sample, samples, d_stats, d_keys);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
