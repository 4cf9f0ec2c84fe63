// delta_reduce.h -- the deterministic two-stage sum of the per-row squared deltas of a half-epoch,
// as device functions: delta_partial_kernel / delta_final_kernel (als_chol.hip) and the fused tail
// kernels of gramian.hip run the SAME loops, so |dP| and |dQ| have the same bits on both paths.
// Workgroups of 256 threads; `sm` = 256 floats of LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lk {

// partial[block] = sum of row_delta over the block's slice (nblocks slices of ceil(n / nblocks))
__device__ __forceinline__ void delta_partial_body(const float *__restrict__ row_delta, int64_t n,
                                                   int nblocks, int block, float *sm,
                                                   float *__restrict__ partial)
{
    const int64_t per = (n + nblocks - 1) / nblocks;
    int64_t b = (int64_t)block * per, e = b + per;
    if (e > n) e = n;
    float s = 0.f;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) s += row_delta[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[block] = sm[0];
}

// out[0] = sqrt(sum of partial[0 .. n))
__device__ __forceinline__ void delta_final_body(const float *__restrict__ partial, int n,
                                                 float *sm, float *__restrict__ out)
{
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sqrtf(sm[0]);
}

}  // namespace lk
