// svd.hip -- the two kernels of the randomized truncated SVD trainer on gfx950
// (`BiasedSVDScorer.train`, src/lenskit/sklearn/svd.py:74-104, which hands the bias residuals to
// sklearn's `TruncatedSVD.fit_transform`; there the work is `randomized_range_finder`'s
// `A @ Q` / `A.T @ Q` products and the normaliser between them).
//
// lk_csr_spmm: sparse x tall-skinny.  out[r][:] = sum over the entries e of CSR row r of
// val[e] * x[idx[e]][:].  A group of G lanes owns a row, lane j holding the float4 chunks j, j + G,
// ... of the panel's row (G = the power of two covering ld / 4 chunks, at most 64: the mapping of
// mf_pairs.hip), so a group reads the 16 G contiguous bytes of x[idx[e]] in one instruction.  The
// group loads G (index, value) pairs at a time, coalesced, and hands them round by shuffles.
//
// Arithmetic.  A row of at most SPMM_SPLIT entries is one fused-multiply-add chain per column, in
// entry order, from zero.  A longer row is cut into segments of SPMM_SPLIT entries; each segment
// is such a chain, and the segments' sums are added in segment order.  The groups of a workgroup
// share the segments of a long row (partial sums through LDS), but which group computed a segment
// changes no bit: the result is a function of the row alone -- not of the grid, the workgroup's
// other rows or the rest of the matrix.  No atomics.
//
// Traffic per pass: nnz * (4 ld + 8) bytes gathered (the panel row, the index, the value; the
// panel -- 19 ... 49 MB at ML-25M -- is served from L2 / Infinity Cache) + n_rows * 4 ld written.
//
// lk_chol_upper_inverse: G = R^T R (R upper), the inverse of R, for the l x l Gramian of a sketch:
// one workgroup, the matrix in LDS (l <= 192) as float32, the sums behind an entry carried in
// float64 and rounded once.  Left-looking Cholesky (thread i owns row i of L = R^T: a chain over
// the columns already done), then thread j solves L x = e_j by forward substitution, keeping x in
// the unused upper triangle.  A pivot that is not positive to working
// precision raises the caller's flag with the caller's step number and is replaced, so that no
// NaN or infinity is ever written.
#include "common.h"

namespace lk {
namespace svd {

constexpr int SPMM_SPLIT = 256;     // entries per chain segment
constexpr int SPMM_THREADS = 256;   // 4 waves
constexpr int CHOL_MAX_L = 192;     // l * (l | 1) + l floats of LDS (145.5 KiB at 192) + 1.5 KiB
constexpr int CHOL_THREADS = 256;

constexpr int UNROLL = 4;

// the lane's chunks of row c of the panel; an index that is no row of it loads nothing
template <int G, int NCH>
__device__ __forceinline__ void load_row(const float *__restrict__ x, int ld_x, int64_t n_cols,
                                         int chunks_in, int j, int32_t c, f32x4 (&xv)[NCH])
{
    const bool ok = c >= 0 && c < n_cols;
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
        const int cc = j + r * G;
        xv[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (ok && cc < chunks_in)
            xv[r] = *reinterpret_cast<const f32x4 *>(x + (int64_t)c * ld_x + 4 * cc);
    }
}

// ... and the next link of the chain (an index that is no row of the panel adds nothing)
template <int G, int NCH>
__device__ __forceinline__ void add_row(int64_t n_cols, int chunks_in, int j, int32_t c, float w,
                                        const f32x4 (&xv)[NCH], f32x4 (&acc)[NCH])
{
    if (c < 0 || c >= n_cols) return;
#pragma unroll
    for (int r = 0; r < NCH; ++r)
        if (j + r * G < chunks_in) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(w, xv[r][q], acc[r][q]);
        }
}

// one chain over the entries [beg, end) of a row, for the lane's chunks
template <int G, int NCH>
__device__ __forceinline__ void chain(const int32_t *__restrict__ idx,
                                      const float *__restrict__ val, int64_t beg, int64_t end,
                                      const float *__restrict__ x, int ld_x, int64_t n_cols,
                                      int chunks_in, int j, f32x4 (&acc)[NCH])
{
#pragma unroll
    for (int r = 0; r < NCH; ++r) acc[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t e0 = beg; e0 < end; e0 += G) {
        int32_t ci = -1;
        float v = 0.0f;
        if (e0 + j < end) {
            ci = idx[e0 + j];
            v = val[e0 + j];
        }
        const int cnt = end - e0 < G ? (int)(end - e0) : G;
        // the lanes of a group run these loops together: the shuffles stay inside the group.
        // Four entries at a time: their panel rows are requested before the first is used.
        int t = 0;
        for (; t + UNROLL <= cnt; t += UNROLL) {
            int32_t c[UNROLL];
            float w[UNROLL];
            f32x4 xv[UNROLL][NCH];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                c[u] = __shfl(ci, t + u, G);
                w[u] = __shfl(v, t + u, G);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                load_row<G, NCH>(x, ld_x, n_cols, chunks_in, j, c[u], xv[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                add_row<G, NCH>(n_cols, chunks_in, j, c[u], w[u], xv[u], acc);
        }
        for (; t < cnt; ++t) {
            const int32_t c = __shfl(ci, t, G);
            const float w = __shfl(v, t, G);
            f32x4 xv[NCH];
            load_row<G, NCH>(x, ld_x, n_cols, chunks_in, j, c, xv);
            add_row<G, NCH>(n_cols, chunks_in, j, c, w, xv, acc);
        }
    }
}

template <bool IS64, int G, int NCH>
__global__ __launch_bounds__(SPMM_THREADS) void csr_spmm_kernel(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ idx,
    const float *__restrict__ val, int64_t n_rows, int64_t n_cols, int64_t nnz,
    const float *__restrict__ x, int ld_x, int l, float *__restrict__ out, int ld_out)
{
    constexpr int NG = SPMM_THREADS / G;  // rows (groups) per workgroup
    constexpr int W = 4 * G * NCH;        // columns a group covers (>= ld_out)
    __shared__ float part[NG * W];        // the segment sums of one round of a long row
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const int chunks_in = (l + 3) / 4, chunks_out = ld_out / 4;
    const int64_t row0 = (int64_t)blockIdx.x * NG;
    f32x4 acc[NCH];

    // the extent of a row; offsets that do not describe entries of this matrix make it empty
    auto extent = [&](int64_t r, int64_t &beg, int64_t &end) {
        beg = end = 0;
        if (r < n_rows) {
            const int64_t b = (int64_t)indptr[r], e = (int64_t)indptr[r + 1];
            if (b >= 0 && b <= e && e <= nnz) {
                beg = b;
                end = e;
            }
        }
    };
    auto store = [&](int64_t r, int cc, const f32x4 &a) {
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = 4 * cc + q < l ? a[q] : 0.0f;  // pad columns: zero
        *reinterpret_cast<f32x4 *>(out + r * ld_out + 4 * cc) = o;
    };

    // rows of at most one segment: one group each
    {
        int64_t beg, end;
        extent(row0 + g, beg, end);
        if (row0 + g < n_rows && end - beg <= SPMM_SPLIT) {
            chain<G, NCH>(idx, val, beg, end, x, ld_x, n_cols, chunks_in, j, acc);
#pragma unroll
            for (int r = 0; r < NCH; ++r)
                if (j + r * G < chunks_out) store(row0 + g, j + r * G, acc[r]);
        }
    }

    // longer rows: the workgroup's groups share the segments, NG of them per round (every
    // condition around a barrier below is the same for the whole workgroup)
    for (int lr = 0; lr < NG; ++lr) {
        int64_t beg, end;
        extent(row0 + lr, beg, end);
        if (end - beg <= SPMM_SPLIT) continue;
        const int64_t segs = (end - beg + SPMM_SPLIT - 1) / SPMM_SPLIT;
        float tot[(W + SPMM_THREADS - 1) / SPMM_THREADS];  // columns threadIdx.x, + 256, ...
#pragma unroll
        for (int m = 0; m < (W + SPMM_THREADS - 1) / SPMM_THREADS; ++m) tot[m] = 0.0f;
        for (int64_t s0 = 0; s0 < segs; s0 += NG) {
            const int64_t s = s0 + g;
            if (s < segs) {
                const int64_t sb = beg + s * SPMM_SPLIT;
                const int64_t se = sb + SPMM_SPLIT < end ? sb + SPMM_SPLIT : end;
                chain<G, NCH>(idx, val, sb, se, x, ld_x, n_cols, chunks_in, j, acc);
#pragma unroll
                for (int r = 0; r < NCH; ++r)
                    *reinterpret_cast<f32x4 *>(&part[g * W + 4 * (j + r * G)]) = acc[r];
            }
            __syncthreads();
            const int live = segs - s0 < NG ? (int)(segs - s0) : NG;
#pragma unroll
            for (int m = 0; m < (W + SPMM_THREADS - 1) / SPMM_THREADS; ++m) {
                const int col = threadIdx.x + m * SPMM_THREADS;
                if (col < W)
                    for (int gg = 0; gg < live; ++gg) tot[m] += part[gg * W + col];  // in order
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < (W + SPMM_THREADS - 1) / SPMM_THREADS; ++m) {
            const int col = threadIdx.x + m * SPMM_THREADS;
            if (col < ld_out) out[(row0 + lr) * ld_out + col] = col < l ? tot[m] : 0.0f;
        }
    }
}

// G = R^T R.  out_lower = L = R^T and out_inv = L^-1 = (R^-1)^T, both [ld_o x ld_o] with zeros
// outside the l x l lower triangle: operands for lk_score_dense as they stand.
__global__ __launch_bounds__(CHOL_THREADS) void chol_upper_inverse_kernel(
    const float *__restrict__ gram, int ld_g, int l, float *__restrict__ out_lower,
    float *__restrict__ out_inv, int ld_o, int *__restrict__ flag, int step)
{
    extern __shared__ float lds[];
    __shared__ double dinv[CHOL_MAX_L];  // 1 / L[j][j]
    __shared__ double pivot;
    const int ls = l | 1;        // odd row stride: the rows of a column fall into different banks
    float *S = lds;              // [l x ls]: lower = L, strictly upper = the inverse, transposed
    float *dg = lds + l * ls;    // [l]: the Gramian's diagonal
    const int tid = threadIdx.x;

    for (int p = tid; p < l * l; p += CHOL_THREADS) {
        const int i = p / l, c = p % l;
        S[i * ls + c] = c <= i ? gram[(int64_t)i * ld_g + c] : 0.0f;
        if (i == c) dg[i] = gram[(int64_t)i * ld_g + c];
    }
    __syncthreads();

    // The entries are float32; the sums behind each of them are carried in float64 (a product of
    // two float32 values is exact there), so an entry is rounded once.  Two interleaved partial
    // sums halve the latency of the chain.
    // A pivot at or below 4 ulp of its diagonal entry is rounding noise: the sketch has lost rank.
    const float tiny = 4.0f * 5.9604644775390625e-8f;
    for (int j = 0; j < l; ++j) {
        const int i = j + tid;  // l <= CHOL_THREADS: one row per thread
        double s = 0.0;
        if (i < l) {
            double s0 = (double)S[i * ls + j], s1 = 0.0;
            int c = 0;
            for (; c + 1 < j; c += 2) {
                s0 = fma(-(double)S[i * ls + c], (double)S[j * ls + c], s0);
                s1 = fma(-(double)S[i * ls + c + 1], (double)S[j * ls + c + 1], s1);
            }
            if (c < j) s0 = fma(-(double)S[i * ls + c], (double)S[j * ls + c], s0);
            s = s0 + s1;
            if (i == j) pivot = s;
        }
        __syncthreads();
        double d = pivot;
        const float gjj = dg[j];
        if (!((float)d > tiny * gjj) || !((float)d < __builtin_inff())) {
            if (tid == 0) atomicCAS(flag, 0, step);  // the first failing step is kept
            d = (gjj > 0.0f && gjj < __builtin_inff()) ? (double)gjj : 1.0;
        }
        const float ljj = (float)sqrt(d);
        if (i < l) {
            const float q = (float)(s / (double)ljj);
            S[i * ls + j] = i == j ? ljj : (q == q && fabsf(q) < __builtin_inff() ? q : 0.0f);
        }
        if (tid == 0) dinv[j] = 1.0 / (double)ljj;
        __syncthreads();
    }

    // column j of L^-1 by forward substitution, kept in row j of the upper triangle
    for (int j = tid; j < l; j += CHOL_THREADS) {
        const float xj = (float)dinv[j];
        for (int i = j + 1; i < l; ++i) {
            double s0 = (double)S[i * ls + j] * (double)xj, s1 = 0.0;
            int c = j + 1;
            for (; c + 1 < i; c += 2) {
                s0 = fma((double)S[i * ls + c], (double)S[j * ls + c], s0);
                s1 = fma((double)S[i * ls + c + 1], (double)S[j * ls + c + 1], s1);
            }
            if (c < i) s0 = fma((double)S[i * ls + c], (double)S[j * ls + c], s0);
            S[j * ls + i] = (float)(-(s0 + s1) * dinv[i]);
        }
    }
    __syncthreads();

    for (int p = tid; p < ld_o * ld_o; p += CHOL_THREADS) {
        const int i = p / ld_o, c = p % ld_o;
        float lo = 0.0f, inv = 0.0f;
        if (i < l && c <= i) {
            lo = S[i * ls + c];
            inv = i == c ? (float)dinv[i] : S[c * ls + i];
        }
        if (out_lower) out_lower[p] = lo;
        out_inv[p] = inv;
    }
}

}  // namespace svd
}  // namespace lk

extern "C" int32_t lk_spmm_split(void) { return lk::svd::SPMM_SPLIT; }

extern "C" int32_t lk_chol_max_l(void) { return lk::svd::CHOL_MAX_L; }

extern "C" int lk_csr_spmm(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                           const float *d_values, int64_t n_rows, int64_t n_cols, int64_t nnz,
                           const float *d_x, int32_t ld_x, int32_t l, float *d_out,
                           int32_t ld_out, void *stream)
{
    using namespace lk::svd;
    LK_REQUIRE(l >= 1 && l <= 1024, "lk_csr_spmm: panel width %d outside 1..1024", l);
    const int padded = (l + 3) / 4 * 4;  // whole float4 chunks are read
    LK_REQUIRE(ld_x >= padded && ld_x % 4 == 0, "lk_csr_spmm: ld_x %d must be a multiple of 4 "
               "covering %d columns", ld_x, padded);
    LK_REQUIRE(ld_out >= padded && ld_out % 4 == 0 && ld_out <= 1024,
               "lk_csr_spmm: ld_out %d must be a multiple of 4 in [%d, 1024]", ld_out, padded);
    LK_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "lk_csr_spmm: bad shape");
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_x && d_out && (nnz == 0 || (d_indices && d_values)),
               "lk_csr_spmm: null pointer");
    LK_REQUIRE(((uintptr_t)d_x | (uintptr_t)d_out) % 16 == 0,
               "lk_csr_spmm: the panels must be 16-byte aligned");
    const int chunks = ld_out / 4;
    int G = 4;
    while (G < 64 && G < chunks) G *= 2;
    const int nch = (chunks + G - 1) / G;
    const int64_t blocks = (n_rows + SPMM_THREADS / G - 1) / (SPMM_THREADS / G);
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_csr_spmm: too many rows");
    const dim3 grid((unsigned)blocks), blk(SPMM_THREADS);
    hipStream_t st = lk::as_stream(stream);
#define LK_SPMM2(IS64, G_, NCH_)                                                                 \
    hipLaunchKernelGGL((csr_spmm_kernel<IS64, G_, NCH_>), grid, blk, 0, st,                      \
                       (const lk::IndPtr<IS64>::type *)d_indptr, d_indices, d_values, n_rows,    \
                       n_cols, nnz, d_x, (int)ld_x, (int)l, d_out, (int)ld_out)
#define LK_SPMM(G_, NCH_)                                                                        \
    do {                                                                                         \
        if (indptr_is_64) LK_SPMM2(true, G_, NCH_);                                              \
        else LK_SPMM2(false, G_, NCH_);                                                          \
    } while (0)
    if (G == 4) LK_SPMM(4, 1);
    else if (G == 8) LK_SPMM(8, 1);
    else if (G == 16) LK_SPMM(16, 1);
    else if (G == 32) LK_SPMM(32, 1);
    else if (nch == 1) LK_SPMM(64, 1);
    else if (nch == 2) LK_SPMM(64, 2);
    else if (nch == 3) LK_SPMM(64, 3);
    else LK_SPMM(64, 4);
#undef LK_SPMM
#undef LK_SPMM2
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_chol_upper_inverse(const float *d_gram, int32_t ld_gram, int32_t l,
                                     float *d_lower, float *d_inverse, int32_t ld_out,
                                     int32_t *d_flag, int32_t step, void *stream)
{
    using namespace lk::svd;
    LK_REQUIRE(l >= 1 && l <= CHOL_MAX_L, "lk_chol_upper_inverse: l = %d outside 1..%d (the "
               "matrix is factored in LDS)", l, CHOL_MAX_L);
    LK_REQUIRE(ld_gram >= l && ld_out >= l, "lk_chol_upper_inverse: leading dimensions (%d, %d) "
               "below l = %d", ld_gram, ld_out, l);
    LK_REQUIRE(step != 0, "lk_chol_upper_inverse: step 0 is the flag's 'no failure'");
    LK_REQUIRE(d_gram && d_inverse && d_flag, "lk_chol_upper_inverse: null pointer");
    const size_t lds = ((size_t)l * (l | 1) + l) * sizeof(float);
    static lk::PerDeviceOnce attr_once;
    bool &attr_set = attr_once.flag();
    if (!attr_set) {
        const size_t most = ((size_t)CHOL_MAX_L * (CHOL_MAX_L | 1) + CHOL_MAX_L) * sizeof(float);
        LK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&chol_upper_inverse_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        attr_set = true;
    }
    hipLaunchKernelGGL(chol_upper_inverse_kernel, dim3(1), dim3(CHOL_THREADS), lds,
                       lk::as_stream(stream), d_gram, (int)ld_gram, (int)l, d_lower, d_inverse,
                       (int)ld_out, d_flag, (int)step);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
