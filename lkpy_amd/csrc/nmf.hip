// nmf.hip -- the coordinate sweep of the NMF trainer on gfx950 (`NMFScorer.train`,
// src/lenskit/sklearn/nmf.py:72-110, which hands the indicator matrix to sklearn's
// `non_negative_factorization`; there the work of one half-iteration is `_update_coordinate_descent`:
// `HHt = Ht^T Ht` (lk_gramian), `XHt = X Ht` (lk_csr_spmm) and `_update_cdnmf_fast`, this file).
//
// lk_nmf_cd_sweep: for every row i of W, the coordinates t = 0 .. k-1 in order:
//     grad = -x[i][t];  grad += HHt[t][r] * W[i][r] for r = 0 .. k-1   (product and sum rounded
//                                                                       separately, in this order)
//     pg   = W[i][t] == 0 ? min(0, grad) : grad;     violation += |pg|
//     W[i][t] = max(W[i][t] - grad / HHt[t][t], 0)   unless HHt[t][t] == 0
// with x = XHt - l1_reg rounded once.  The rows are independent, so this is sklearn's loop (which
// runs t outside and i inside) row by row, and W has the bits of that loop in float32.
//
// Layout.  One row per lane, one wave of 64 rows per workgroup.  HHt [k x k] sits in LDS and is
// read as a broadcast (every lane the same address).  The workgroup's tiles of W and of x are
// staged through LDS with the odd row pitch KP + 1: the row-major panels are read and written
// coalesced, and the lanes then walk their own rows without bank conflicts.  LDS: 4 (k^2 +
// 2 * 64 (KP + 1)) bytes -- 130 KiB at k = 128, 49 KiB at k = 64.
//
// The violation is a float64 sum: a lane adds its |pg| in coordinate order, lane 0 adds the 64
// lanes' sums in lane order, and a second one-workgroup kernel adds the workgroups' sums (thread
// j the partials j, j + 256, ... in order, then a fixed tree).  No floating-point atomics: the
// value is a function of the panels alone.
#include "common.h"

namespace lk {
namespace nmf {

constexpr int MAX_K = 128;
constexpr int ROWS = 64;           // rows per workgroup: one wave, one row per lane
constexpr int FINAL_THREADS = 256;

__global__ __launch_bounds__(ROWS) void cd_sweep_kernel(
    float *__restrict__ w, int64_t n, int k, int kp, const float *__restrict__ hht, int ld_h,
    const float *__restrict__ xht, float l1_reg, double *__restrict__ partial)
{
    // sklearn's loop rounds the product, then the sum.  The compiler's default contracts
    // a * b + c into one fused multiply-add -- through the inlined __fmul_rn / __fadd_rn too,
    // whose instructions carry their header's permission to contract -- so the arithmetic of this
    // kernel is written with plain operators under a pragma that withholds it.
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    __shared__ double lane_sum[ROWS];
    const int pitch = kp + 1;
    float *H = lds;                  // [k x k]
    float *Wt = lds + k * k;         // [ROWS x pitch]
    float *Xt = Wt + ROWS * pitch;   // [ROWS x pitch]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int rows = n - row0 < ROWS ? (int)(n - row0) : ROWS;

    for (int p = tid; p < k * k; p += ROWS) H[p] = hht[(int64_t)(p / k) * ld_h + p % k];
    for (int p = tid; p < rows * kp; p += ROWS) {
        const int r = p / kp, c = p % kp;
        Wt[r * pitch + c] = w[row0 * kp + p];
        Xt[r * pitch + c] = xht[row0 * kp + p] - l1_reg;
    }
    __syncthreads();

    double viol = 0.0;
    if (tid < rows) {
        float *wr = Wt + tid * pitch;
        const float *xr = Xt + tid * pitch;
        for (int t = 0; t < k; ++t) {
            const float *hr = H + t * k;
            float grad = -xr[t];
            for (int r = 0; r < k; ++r) {
                const float prod = hr[r] * wr[r];
                grad = grad + prod;
            }
            const float wt = wr[t];
            const float pg = wt == 0.0f ? (grad < 0.0f ? grad : 0.0f) : grad;
            viol += (double)fabsf(pg);
            const float hess = hr[t];
            if (hess != 0.0f) {
                const float v = wt - grad / hess;  // (IEEE division: no fast-math flag is set)
                wr[t] = v > 0.0f ? v : 0.0f;
            }
        }
    }
    lane_sum[tid] = viol;
    __syncthreads();

    for (int p = tid; p < rows * kp; p += ROWS) {
        const int r = p / kp, c = p % kp;
        w[row0 * kp + p] = c < k ? Wt[r * pitch + c] : 0.0f;  // pad columns stay zero
    }
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < ROWS; ++j) s += lane_sum[j];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(FINAL_THREADS) void violation_final_kernel(
    const double *__restrict__ partial, int64_t n, double *__restrict__ out)
{
    __shared__ double sm[FINAL_THREADS];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FINAL_THREADS) s += partial[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = FINAL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}

static size_t sweep_lds_bytes(int k, int kp)
{
    return ((size_t)k * k + 2 * (size_t)ROWS * (kp + 1)) * sizeof(float);
}

}  // namespace nmf
}  // namespace lk

extern "C" int32_t lk_nmf_max_k(void) { return lk::nmf::MAX_K; }

extern "C" size_t lk_nmf_workspace_bytes(int64_t n)
{
    using namespace lk::nmf;
    const int64_t blocks = n > 0 ? (n + ROWS - 1) / ROWS : 1;
    return (size_t)blocks * sizeof(double);
}

extern "C" int lk_nmf_cd_sweep(float *d_w, int64_t n, int32_t k, int32_t ld, const float *d_hht,
                               int32_t ld_hht, const float *d_xht, float l1_reg,
                               double *d_violation, void *d_ws, void *stream)
{
    using namespace lk::nmf;
    LK_REQUIRE(k >= 1 && k <= MAX_K, "lk_nmf_cd_sweep: k = %d outside 1..%d (lk_nmf_max_k)", k,
               MAX_K);
    const int KP = lk_padded_dim(k);
    LK_REQUIRE(ld == KP, "lk_nmf_cd_sweep: ld=%d must equal lk_padded_dim(k)=%d", ld, KP);
    LK_REQUIRE(ld_hht >= k, "lk_nmf_cd_sweep: ld_hht=%d < k=%d", ld_hht, k);
    LK_REQUIRE(n >= 0, "lk_nmf_cd_sweep: negative n");
    LK_REQUIRE(d_violation && d_ws, "lk_nmf_cd_sweep: null pointer");
    LK_REQUIRE(n == 0 || (d_w && d_hht && d_xht), "lk_nmf_cd_sweep: null pointer");
    const int64_t blocks = (n + ROWS - 1) / ROWS;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_nmf_cd_sweep: too many rows");
    hipStream_t st = lk::as_stream(stream);
    double *partial = static_cast<double *>(d_ws);
    if (blocks > 0) {
        static lk::PerDeviceOnce attr_once;
        bool &attr_set = attr_once.flag();
        if (!attr_set) {
            LK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cd_sweep_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)sweep_lds_bytes(MAX_K, MAX_K)));
            attr_set = true;
        }
        hipLaunchKernelGGL(cd_sweep_kernel, dim3((unsigned)blocks), dim3(ROWS),
                           sweep_lds_bytes(k, KP), st, d_w, n, (int)k, KP, d_hht, (int)ld_hht,
                           d_xht, l1_reg, partial);
        LK_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(violation_final_kernel, dim3(1), dim3(FINAL_THREADS), 0, st, partial,
                       blocks, d_violation);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
