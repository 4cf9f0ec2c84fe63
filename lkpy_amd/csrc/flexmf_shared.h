// flexmf_shared.h -- what the minibatch trainers (flexmf.hip, lightgcn.hip) share: the
// hyper-parameters as the kernels use them, the logistic functions, Torch's AdamW update of one
// element, the batch-loss kernel and the scratch carving of a step.
#pragma once

#include <math.h>

#include "common.h"

namespace lk {
namespace fx {

struct Scalars {  // the hyper-parameters as the kernels use them (float32 where Torch rounds)
    int loss, l2, n_neg;
    float pos_weight, reg;
    // SparseAdam
    float omb1, omb2, eps, sparse_step;
    // AdamW
    float decay, beta2, adamw_step, bc2_sqrt;
};

__device__ __forceinline__ float softplusf(float x)
{
    return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf(float x)
{
    if (x >= 0.0f) return 1.0f / (1.0f + expf(-x));
    const float e = expf(x);
    return e / (1.0f + e);
}

// the batch loss: one workgroup, a fixed order
static __global__ __launch_bounds__(256) void flexmf_loss_kernel(const float *__restrict__ lossv,
                                                                 int64_t B,
                                                                 float *__restrict__ loss,
                                                                 float *__restrict__ loss_sum)
{
    __shared__ double part[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < B; i += 256) s += (double)lossv[i];
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const float l = (float)part[0];
        *loss = l;
        if (loss_sum) *loss_sum += l;
    }
}

__device__ __forceinline__ void adamw(float &x, float &m, float &v, float g, const Scalars &H)
{
    // torch.optim.adam._single_tensor_adam with decoupled weight decay
    x = x * H.decay;
    m = m + H.omb1 * (g - m);            // lerp_(grad, 1 - beta1), weight < 0.5
    v = v * H.beta2 + H.omb2 * (g * g);  // mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) / H.bc2_sqrt + H.eps;
    x = x + (-H.adamw_step) * m / denom;
}

static size_t carve(char *base, size_t &off, size_t bytes, void **out)
{
    if (base) *out = base + off;
    off += align_up(bytes ? bytes : 1, 256);
    return off;
}

static int bits_for(int64_t n)
{
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return b;
}

// the hyper-parameters rounded to float32 where Torch's optimisers round them
static Scalars scalars_of(const lk_flexmf_hyper &h)
{
    Scalars H{};
    H.loss = h.loss;
    H.l2 = h.l2 ? 1 : 0;
    H.n_neg = h.n_neg;
    H.pos_weight = (float)h.pos_weight;
    H.reg = (float)h.reg;
    H.omb1 = (float)(1.0 - h.beta1);
    H.omb2 = (float)(1.0 - h.beta2);
    H.eps = (float)h.eps;
    H.sparse_step = (float)(h.lr * sqrt(h.bias_corr2) / h.bias_corr1);
    H.decay = (float)(1.0 - h.lr * h.reg);
    H.beta2 = (float)h.beta2;
    H.adamw_step = (float)(h.lr / h.bias_corr1);
    H.bc2_sqrt = (float)sqrt(h.bias_corr2);
    return H;
}

}  // namespace fx
}  // namespace lk
