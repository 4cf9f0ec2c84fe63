// stochastic_shared.h -- what the key kernels of the stochastic ranker share (stochastic.hip: whole
// panels of score rows; ragged_stochastic.hip: ragged candidate lists): the key function and its
// constants, the weight of an entry under each transform, the terms of a row's sum and the
// workgroup reduction whose order both must keep.  Both kernels inline THESE expressions, so an
// entry has the same bits wherever it is computed.
#pragma once

#include <float.h>
#include <math.h>

#include "common.h"
#include "philox.h"

namespace lk {
namespace stoch {

constexpr float LOG_FLT_MIN = -87.33654475055310898657f;  // log(2^-126)

// log(-log u) for the uniform of the random word `bits`
__device__ __forceinline__ float log_neg_log_u(uint32_t bits)
{
    const float u = (float)(2u * (bits >> 9) + 1u) * 0x1p-24f;  // odd 24-bit integer: exact
    const float nl = u > 0.5f ? -log1pf(-(1.0f - u)) : -logf(u);
    return logf(nl);
}

__device__ __forceinline__ float key_of(float logw, uint32_t bits)
{
    return fmaxf(logw, LOG_FLT_MIN) - log_neg_log_u(bits);
}

__device__ __forceinline__ float log_of_weight(float w)
{
    return w >= FLT_MIN ? logf(w) : LOG_FLT_MIN;  // (negative, zero and subnormal: the clamp)
}

// workgroup reductions with one fixed order: butterfly inside the wave (every lane ends with the
// same bits), the waves' values in wave order through LDS
template <int BLK, class Op>
__device__ __forceinline__ float block_reduce(float v, float *lds, Op op)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    if constexpr (BLK > WAVE) {
        __syncthreads();  // (the previous reduction's reads of lds are over)
        if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < BLK / WAVE; ++w) v = op(v, lds[w]);
    }
    return v;
}

struct OpMax {
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct OpMin {
    __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct OpAdd {
    __device__ float operator()(float a, float b) const { return a + b; }
};

// the threads of a row's statistics workgroup: a wave for short rows, a workgroup for long ones --
// chosen by the row length alone, so a row reduces in the same order in every batch
constexpr int64_t STATS_WAVE_MAX = 2048;
constexpr int STATS_BLK_LONG = 256;

// does the row's sum exist under this transform?  (none: 0; linear over one value: 0)
__device__ __forceinline__ bool has_sum(int transform, float range)
{
    return transform == LK_STOCHASTIC_SOFTMAX || (transform == LK_STOCHASTIC_LINEAR && range > 0.f);
}

// the term a participating entry adds to the row's sum (has_sum)
__device__ __forceinline__ float sum_term(float score, float scale, float mx, float mn,
                                          float range, int transform)
{
    const float x = score * scale;
    return transform == LK_STOCHASTIC_SOFTMAX ? expf(x - mx) : (x - mn) / range;
}

// linear: every weight is 1/N when the row holds one value or its terms sum to 0
__device__ __forceinline__ bool uniform_weights(float range, float sum)
{
    return !(range > 0.f) || !(sum > 0.f);
}

// log w of an entry that takes part; `log_sum` = log(sum) (softmax), `log_unif` = -log N
__device__ __forceinline__ float log_weight(float score, float scale, float mx, float mn,
                                            float range, float sum, bool uniform, float log_sum,
                                            float log_unif, int transform)
{
    const float x = score * scale;
    float logw;
    if (transform == LK_STOCHASTIC_SOFTMAX) logw = (x - mx) - log_sum;
    else if (transform == LK_STOCHASTIC_LINEAR)
        logw = uniform ? log_unif : log_of_weight(((x - mn) / range) / sum);
    else logw = log_of_weight(x);
    return logw;
}

inline bool bad_transform(int t)
{
    return t != LK_STOCHASTIC_NONE && t != LK_STOCHASTIC_SOFTMAX && t != LK_STOCHASTIC_LINEAR;
}

}  // namespace stoch
}  // namespace lk
