// ragged.h -- what the kernels over ragged per-query target lists share (candidates.hip,
// sparse_candidates.hip): query q owns the positions [ptr[q], ptr[q + 1]) of one flat array.
#pragma once
#include "common.h"

namespace lk {
namespace ragged {

__device__ __forceinline__ int64_t clampi(int64_t v, int64_t lo, int64_t hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// the query q with ptr[q] <= pos < ptr[q + 1] (offsets ascending from 0, pos < ptr[n]); always in
// [0, n - 1], whatever the offsets hold
__device__ __forceinline__ int64_t query_of(const int64_t *__restrict__ ptr, int64_t n, int64_t pos)
{
    int64_t lo = 0, hi = n;  // ptr[lo] <= pos < ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace ragged
}  // namespace lk
