// hpf.hip -- the four kernels of the hierarchical Poisson factorization trainer on gfx950
// (`HPFScorer.train`, src/lenskit/hpf.py:81-100, which hands the count matrix to `hpfrec.HPF.fit`;
// the algorithm is coordinate-ascent variational inference: Gopalan, Hofman, Blei 2015,
// Algorithm 1).
//
// One iteration: E = psi(shp) - log(rte) for both sides (lk_hpf_expect_log), the shape sums of
// the users over Y and of the items over Y^T (lk_hpf_shape_pass, twice), then the rates, the
// means and the column sums of the users and of the items (lk_hpf_rates, twice).
// lk_hpf_loglik_rows serves the stopping check.
//
// lk_hpf_shape_pass is lk_csr_spmm's gather with a softmax in the middle.  A group of G lanes owns
// a row, lane j holding the float4 chunk j of the row's E (G = the power of two covering ld / 4
// chunks, at most 64: ld <= 256), which stays in registers for the whole chain.  The group loads
// G (index, value) pairs at a time, coalesced, hands them round by shuffles and requests four
// rows of the other side's E before the first is used.  Per entry: s = E_row + E_col, m = max s,
// p = exp(s - m), Z = sum p, acc = fma(y / Z, p, acc).  The two reductions stay inside the group:
// the lane's four values in column order, then an xor butterfly over the G lanes (DPP row
// operations below 16 lanes, shuffles above) -- both operands of every addition are the same two
// numbers in both lanes, so all lanes hold the same bits and the order depends on G alone.
//
// Arithmetic of the sums: lk_csr_spmm's contract.  A row of at most SPMM_SPLIT entries is one
// fused-multiply-add chain per column, in entry order, from zero; a longer row is cut into
// segments of that length, added in segment order; the prior is added last.  Each entry's weights
// are computed again in the pass over the transposed matrix: no atomics, and a row's result is a
// function of the row alone.
//
// Traffic per pass: nnz * (4 ld + 8) bytes gathered + n_rows * 8 ld for the row operand and the
// result.
#include "common.h"

namespace lk {
namespace hpf {

constexpr int SPLIT = 256;         // entries per chain segment: lk_spmm_split()
constexpr int THREADS = 256;       // 4 waves
constexpr int UNROLL = 4;
constexpr int RATES_BLOCK = 256;   // rows behind one partial column sum: a constant of the file
constexpr int RATES_TILE = 32;     // rows of a block held in LDS at a time
constexpr int MAX_LD = LK_FLEXMF_MAX_K;
constexpr int LL_LONG = 1024;      // log-likelihood: rows beyond this are shared by a workgroup,
constexpr int LL_SEG = 64;         // each group turning this many entries into terms per round

// ---- E = psi(shp) - log(rte) ---------------------------------------------------------------
// digamma in float64: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6, then the
// asymptotic series up to x^-16 (the first omitted term is below 1e-14 there)
__device__ __forceinline__ double digamma(double x)
{
    double r = 0.0;
    while (x < 6.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    double s = 3617.0 / 8160.0;
    s = fma(s, i2, -1.0 / 12.0);
    s = fma(s, i2, 691.0 / 32760.0);
    s = fma(s, i2, -1.0 / 132.0);
    s = fma(s, i2, 1.0 / 240.0);
    s = fma(s, i2, -1.0 / 252.0);
    s = fma(s, i2, 1.0 / 120.0);
    s = fma(s, i2, -1.0 / 12.0);
    return r + (log(x) - 0.5 * i + s * i2);
}

__global__ __launch_bounds__(THREADS) void expect_log_kernel(const float *__restrict__ shp,
                                                             const float *__restrict__ rte,
                                                             int64_t n, int k, int ld,
                                                             float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (p >= n * ld) return;
    const int c = (int)(p % ld);
    float e = 0.0f;  // pad columns: zero
    if (c < k) e = (float)(digamma((double)shp[p]) - log((double)rte[p]));
    out[p] = e;
}

// ---- the shape pass --------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    const int x = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false));
}

// the partner's value at every level of a butterfly over G lanes.  Below 16 lanes the partner is
// reached by DPP: quad_perm [1 0 3 2], quad_perm [2 3 0 1], then row_half_mirror and row_mirror
// (lane i of 8 / 16 reads lane 7 - i / 15 - i: after the two quad levels every lane of a quad
// holds the quad's value, so any lane of the other quad / the other half serves).
template <int G, typename OP>
__device__ __forceinline__ float group_reduce(float v, OP op)
{
    v = op(v, dpp<0xB1>(v));
    v = op(v, dpp<0x4E>(v));
    if (G >= 8) v = op(v, dpp<0x141>(v));
    if (G >= 16) v = op(v, dpp<0x140>(v));
    if (G >= 32) v = op(v, __shfl_xor(v, 16, 64));
    if (G >= 64) v = op(v, __shfl_xor(v, 32, 64));
    return v;
}

// the lane's chunk of row c of the other side's E; an index that is no row of it loads zeros
__device__ __forceinline__ f32x4 load_chunk(const float *__restrict__ x, int ld, int64_t n_cols,
                                            int chunks, int j, int32_t c)
{
    f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (c >= 0 && c < n_cols && j < chunks)
        v = *reinterpret_cast<const f32x4 *>(x + (int64_t)c * ld + 4 * j);
    return v;
}

// one entry: the softmax over the k components and the next link of the chain.  Every lane of
// the group runs it (the reductions need them all); an index that is no column of the matrix has
// the weight zero, which leaves acc as it is.
template <int G>
__device__ __forceinline__ void add_entry(int64_t n_cols, int k, int j, int32_t c, float y,
                                          const f32x4 &er, const f32x4 &ec, f32x4 &acc)
{
    const float ninf = -__builtin_inff();
    float s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = 4 * j + q < k ? er[q] + ec[q] : ninf;
    float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    m = group_reduce<G>(m, [](float a, float b) { return fmaxf(a, b); });
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = 4 * j + q < k ? expf(s[q] - m) : 0.0f;  // underflow: 0
    float z = (p[0] + p[1]) + (p[2] + p[3]);
    z = group_reduce<G>(z, [](float a, float b) { return a + b; });  // >= 1: the maximum's term
    const float w = (c >= 0 && c < n_cols) ? y / z : 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = fmaf(w, p[q], acc[q]);
}

// one chain over the entries [beg, end) of a row, for the lane's chunk
template <int G>
__device__ __forceinline__ void chain(const int32_t *__restrict__ idx,
                                      const float *__restrict__ val, int64_t beg, int64_t end,
                                      const float *__restrict__ x, int ld, int64_t n_cols, int k,
                                      int chunks, int j, const f32x4 &er, f32x4 &acc)
{
    acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t e0 = beg; e0 < end; e0 += G) {
        int32_t ci = -1;
        float v = 0.0f;
        if (e0 + j < end) {
            ci = idx[e0 + j];
            v = val[e0 + j];
        }
        const int cnt = end - e0 < G ? (int)(end - e0) : G;
        // the lanes of a group run these loops together: the shuffles stay inside the group
        int t = 0;
        for (; t + UNROLL <= cnt; t += UNROLL) {
            int32_t c[UNROLL];
            float y[UNROLL];
            f32x4 ec[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                c[u] = __shfl(ci, t + u, G);
                y[u] = __shfl(v, t + u, G);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) ec[u] = load_chunk(x, ld, n_cols, chunks, j, c[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) add_entry<G>(n_cols, k, j, c[u], y[u], er, ec[u], acc);
        }
        for (; t < cnt; ++t) {
            const int32_t c = __shfl(ci, t, G);
            const float y = __shfl(v, t, G);
            const f32x4 ec = load_chunk(x, ld, n_cols, chunks, j, c);
            add_entry<G>(n_cols, k, j, c, y, er, ec, acc);
        }
    }
}

template <bool IS64, int G>
__global__ __launch_bounds__(THREADS) void shape_pass_kernel(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ idx,
    const float *__restrict__ val, int64_t n_rows, int64_t n_cols, int64_t nnz,
    const float *__restrict__ e_rows, const float *__restrict__ e_cols, int k, int ld, float prior,
    float *__restrict__ out)
{
    constexpr int NG = THREADS / G;  // rows (groups) per workgroup
    constexpr int W = 4 * G;         // columns a group covers (>= ld)
    __shared__ float part[NG * W];   // the segment sums of one round of a long row
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const int chunks = ld / 4;
    const int64_t row0 = (int64_t)blockIdx.x * NG;
    f32x4 acc;

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
    auto row_operand = [&](int64_t r) {
        f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (r < n_rows && j < chunks) v = *reinterpret_cast<const f32x4 *>(e_rows + r * ld + 4 * j);
        return v;
    };

    // rows of at most one segment: one group each
    {
        int64_t beg, end;
        extent(row0 + g, beg, end);
        if (row0 + g < n_rows && end - beg <= SPLIT) {
            const f32x4 er = row_operand(row0 + g);
            chain<G>(idx, val, beg, end, e_cols, ld, n_cols, k, chunks, j, er, acc);
            if (j < chunks) {
                f32x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = 4 * j + q < k ? prior + acc[q] : 0.0f;
                *reinterpret_cast<f32x4 *>(out + (row0 + g) * ld + 4 * j) = o;
            }
        }
    }

    // longer rows: the workgroup's groups share the segments, NG of them per round (every
    // condition around a barrier below is the same for the whole workgroup)
    for (int lr = 0; lr < NG; ++lr) {
        int64_t beg, end;
        extent(row0 + lr, beg, end);
        if (end - beg <= SPLIT) continue;
        const int64_t segs = (end - beg + SPLIT - 1) / SPLIT;
        const f32x4 er = row_operand(row0 + lr);
        float tot = 0.0f;  // column threadIdx.x (W <= THREADS)
        for (int64_t s0 = 0; s0 < segs; s0 += NG) {
            const int64_t s = s0 + g;
            if (s < segs) {
                const int64_t sb = beg + s * SPLIT;
                const int64_t se = sb + SPLIT < end ? sb + SPLIT : end;
                chain<G>(idx, val, sb, se, e_cols, ld, n_cols, k, chunks, j, er, acc);
                *reinterpret_cast<f32x4 *>(&part[g * W + 4 * j]) = acc;
            }
            __syncthreads();
            const int live = segs - s0 < NG ? (int)(segs - s0) : NG;
            if (threadIdx.x < W)
                for (int gg = 0; gg < live; ++gg) tot += part[gg * W + threadIdx.x];  // in order
            __syncthreads();
        }
        if (threadIdx.x < ld)
            out[(row0 + lr) * ld + threadIdx.x] = threadIdx.x < k ? prior + tot : 0.0f;
    }
}

// ---- rates, means, hyper-rates and column sums of one side ------------------------------------
// A workgroup owns RATES_BLOCK rows, RATES_TILE of them at a time: a group of G lanes per row
// forms the row's rates and means (coalesced), the means go through LDS, one thread per row adds
// them in column order and one thread per column adds them in row order, both in float64.
__global__ __launch_bounds__(THREADS) void rates_kernel(
    const float *__restrict__ shp, int64_t n, int k, int ld, float shp_hyper, double prior_ratio,
    float *__restrict__ hyper_rte, const float *__restrict__ other_colsum, float *__restrict__ rte,
    float *__restrict__ mean, double *__restrict__ partial)
{
    __shared__ float tile[RATES_TILE * MAX_LD];
    const int chunks = ld / 4;  // lanes per row
    const int rows_per_step = THREADS / chunks;
    const int g = threadIdx.x / chunks, j = threadIdx.x % chunks;
    const int64_t row0 = (int64_t)blockIdx.x * RATES_BLOCK;
    f32x4 other = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * j + q < k) other[q] = other_colsum[4 * j + q];
    double colsum = 0.0;  // column threadIdx.x over the block's rows, in row order
    for (int t0 = 0; t0 < RATES_BLOCK && row0 + t0 < n; t0 += RATES_TILE) {
        // (the threads left over when ld / 4 does not divide the workgroup form no group)
        for (int lr = g < rows_per_step ? g : RATES_TILE; lr < RATES_TILE; lr += rows_per_step) {
            const int64_t r = row0 + t0 + lr;
            f32x4 mu = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (r < n) {
                const f32x4 s = *reinterpret_cast<const f32x4 *>(shp + r * ld + 4 * j);
                const float base = shp_hyper / hyper_rte[r];
                f32x4 rt = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (4 * j + q < k) {
                        rt[q] = base + other[q];
                        mu[q] = s[q] / rt[q];
                    }
                *reinterpret_cast<f32x4 *>(rte + r * ld + 4 * j) = rt;
                *reinterpret_cast<f32x4 *>(mean + r * ld + 4 * j) = mu;
            }
            *reinterpret_cast<f32x4 *>(&tile[lr * ld + 4 * j]) = mu;
        }
        __syncthreads();  // (also orders the reads of hyper_rte above before the writes below)
        if (threadIdx.x < RATES_TILE && row0 + t0 + threadIdx.x < n) {
            double s = 0.0;
            for (int c = 0; c < k; ++c) s += (double)tile[threadIdx.x * ld + c];
            hyper_rte[row0 + t0 + threadIdx.x] = (float)(prior_ratio + s);
        }
        if (threadIdx.x < k)
            for (int lr = 0; lr < RATES_TILE; ++lr) colsum += (double)tile[lr * ld + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < k) partial[(int64_t)blockIdx.x * k + threadIdx.x] = colsum;
}

// the partial sums of the blocks, added in block order
__global__ __launch_bounds__(THREADS) void rates_colsum_kernel(const double *__restrict__ partial,
                                                               int64_t blocks, int k,
                                                               float *__restrict__ colsum)
{
    if ((int)threadIdx.x >= k) return;
    double s = 0.0;
    for (int64_t b = 0; b < blocks; ++b) s += partial[b * k + threadIdx.x];
    colsum[threadIdx.x] = (float)s;
}

// ---- the data term of the log-likelihood, per row ----------------------------------------------
__device__ __forceinline__ double group_sum_f64(double v, int G)
{
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The terms y_e log(theta_r . beta[col_e]) of the entries [beg, end) of a row, G at a time: the
// group forms the G inner products together (float64, a butterfly over its lanes), lane t keeps
// that of entry e0 + t and takes one logarithm, and sink(e0, cnt, term) receives the batch --
// lane t holding the term of entry e0 + t, zero where there is no entry or its index is no column.
template <int G, typename SINK>
__device__ __forceinline__ void loglik_terms(const int32_t *__restrict__ idx,
                                             const float *__restrict__ val, int64_t beg,
                                             int64_t end, const float *__restrict__ beta, int ld,
                                             int64_t n_cols, int k, int chunks, int j,
                                             const f32x4 &th, SINK sink)
{
    for (int64_t e0 = beg; e0 < end; e0 += G) {
        int32_t ci = -1;
        float v = 0.0f;
        if (e0 + j < end) {
            ci = idx[e0 + j];
            v = val[e0 + j];
        }
        const int cnt = end - e0 < G ? (int)(end - e0) : G;
        double mine = 1.0;
        for (int t0 = 0; t0 < cnt; t0 += UNROLL) {
            f32x4 b[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int32_t c = t0 + u < cnt ? __shfl(ci, t0 + u, G) : -1;
                b[u] = load_chunk(beta, ld, n_cols, chunks, j, c);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                double d = 0.0;  // pad columns are zero on both sides
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (4 * j + q < k) d = fma((double)th[q], (double)b[u][q], d);
                d = group_sum_f64(d, G);
                if (t0 + u == j) mine = d;
            }
        }
        const bool have = j < cnt && ci >= 0 && ci < n_cols;
        sink(e0, cnt, have ? (double)v * log(mine) : 0.0);
    }
}

template <bool IS64, int G>
__global__ __launch_bounds__(THREADS) void loglik_rows_kernel(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ idx,
    const float *__restrict__ val, int64_t n_rows, int64_t n_cols, int64_t nnz,
    const float *__restrict__ theta, const float *__restrict__ beta, int k, int ld,
    double *__restrict__ out)
{
    constexpr int NG = THREADS / G;
    __shared__ double terms[NG * LL_SEG];  // the terms of one round of a long row, in entry order
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const int chunks = ld / 4;
    const int64_t row0 = (int64_t)blockIdx.x * NG;

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
    auto row_operand = [&](int64_t r) {
        f32x4 v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (j < chunks) v = *reinterpret_cast<const f32x4 *>(theta + r * ld + 4 * j);
        return v;
    };

    // rows of at most LL_LONG entries: one group each, the terms added as they come
    {
        int64_t beg, end;
        extent(row0 + g, beg, end);
        if (row0 + g < n_rows && end - beg <= LL_LONG) {
            double sum = 0.0;
            loglik_terms<G>(idx, val, beg, end, beta, ld, n_cols, k, chunks, j,
                            row_operand(row0 + g), [&](int64_t, int cnt, double term) {
                                for (int t = 0; t < cnt; ++t) sum += __shfl(term, t, G);
                            });
            if (j == 0) out[row0 + g] = sum;
        }
    }

    // longer rows: the workgroup's groups form the terms of NG * LL_SEG consecutive entries per
    // round, one thread adds them in entry order (every condition around a barrier below is the
    // same for the whole workgroup)
    for (int lr = 0; lr < NG; ++lr) {
        int64_t beg, end;
        extent(row0 + lr, beg, end);
        if (end - beg <= LL_LONG) continue;
        const f32x4 th = row_operand(row0 + lr);
        double tot = 0.0;
        for (int64_t s0 = beg; s0 < end; s0 += NG * LL_SEG) {
            const int64_t sb = s0 + (int64_t)g * LL_SEG;
            const int64_t se = sb + LL_SEG < end ? sb + LL_SEG : end;
            if (sb < end)
                loglik_terms<G>(idx, val, sb, se, beta, ld, n_cols, k, chunks, j, th,
                                [&](int64_t e0, int cnt, double term) {
                                    if (j < cnt) terms[e0 - s0 + j] = term;
                                });
            __syncthreads();
            const int live = end - s0 < NG * LL_SEG ? (int)(end - s0) : NG * LL_SEG;
            if (threadIdx.x == 0) {
#pragma unroll 8
                for (int i = 0; i < live; ++i) tot += terms[i];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) out[row0 + lr] = tot;
    }
}

static int check_panel(const char *who, int k, int ld)
{
    LK_REQUIRE(k >= 1 && k <= LK_FLEXMF_MAX_K, "%s: embedding size %d outside 1..%d", who, k,
               LK_FLEXMF_MAX_K);
    LK_REQUIRE(ld % 4 == 0 && ld >= (k + 3) / 4 * 4 && ld <= MAX_LD,
               "%s: ld %d must be a multiple of 4 in [%d, %d]", who, ld, (k + 3) / 4 * 4, MAX_LD);
    return LK_OK;
}

static int group_lanes(int ld)
{
    int G = 4;
    while (G < 64 && G < ld / 4) G *= 2;
    return G;
}

}  // namespace hpf
}  // namespace lk

extern "C" int32_t lk_hpf_rates_block(void) { return lk::hpf::RATES_BLOCK; }

extern "C" int lk_hpf_expect_log(const float *d_shp, const float *d_rte, int64_t n, int32_t k,
                                 int32_t ld, float *d_out, void *stream)
{
    using namespace lk::hpf;
    if (int rc = check_panel("lk_hpf_expect_log", k, ld)) return rc;
    LK_REQUIRE(n >= 0, "lk_hpf_expect_log: bad shape");
    if (n == 0) return LK_OK;
    LK_REQUIRE(d_shp && d_rte && d_out, "lk_hpf_expect_log: null pointer");
    const int64_t blocks = (n * ld + THREADS - 1) / THREADS;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_hpf_expect_log: too many rows");
    hipLaunchKernelGGL(expect_log_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                       lk::as_stream(stream), d_shp, d_rte, n, (int)k, (int)ld, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_hpf_shape_pass(const void *d_indptr, int indptr_is_64, const int32_t *d_indices,
                                 const float *d_values, int64_t n_rows, int64_t n_cols,
                                 int64_t nnz, const float *d_e_rows, const float *d_e_cols,
                                 int32_t k, int32_t ld, float prior, float *d_out, void *stream)
{
    using namespace lk::hpf;
    if (int rc = check_panel("lk_hpf_shape_pass", k, ld)) return rc;
    LK_REQUIRE(lk_spmm_split() == SPLIT, "lk_hpf_shape_pass: the segment length %d is not "
               "lk_spmm_split() = %d", SPLIT, lk_spmm_split());
    LK_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "lk_hpf_shape_pass: bad shape");
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_e_rows && d_out && (n_cols == 0 || d_e_cols) &&
               (nnz == 0 || (d_indices && d_values)), "lk_hpf_shape_pass: null pointer");
    LK_REQUIRE(((uintptr_t)d_e_rows | (uintptr_t)d_e_cols | (uintptr_t)d_out) % 16 == 0,
               "lk_hpf_shape_pass: the panels must be 16-byte aligned");
    LK_REQUIRE(d_out != d_e_rows && d_out != d_e_cols,
               "lk_hpf_shape_pass: the result must not alias an operand");
    const int G = group_lanes(ld);
    const int64_t blocks = (n_rows + THREADS / G - 1) / (THREADS / G);
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_hpf_shape_pass: too many rows");
    const dim3 grid((unsigned)blocks), blk(THREADS);
    hipStream_t st = lk::as_stream(stream);
#define LK_HPF2(IS64, G_)                                                                        \
    hipLaunchKernelGGL((shape_pass_kernel<IS64, G_>), grid, blk, 0, st,                          \
                       (const lk::IndPtr<IS64>::type *)d_indptr, d_indices, d_values, n_rows,    \
                       n_cols, nnz, d_e_rows, d_e_cols, (int)k, (int)ld, prior, d_out)
#define LK_HPF(G_)                                                                               \
    do {                                                                                         \
        if (indptr_is_64) LK_HPF2(true, G_);                                                     \
        else LK_HPF2(false, G_);                                                                 \
    } while (0)
    if (G == 4) LK_HPF(4);
    else if (G == 8) LK_HPF(8);
    else if (G == 16) LK_HPF(16);
    else if (G == 32) LK_HPF(32);
    else LK_HPF(64);
#undef LK_HPF
#undef LK_HPF2
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" size_t lk_hpf_rates_workspace_bytes(int64_t n, int32_t k)
{
    using namespace lk::hpf;
    if (n < 0 || k < 1 || k > LK_FLEXMF_MAX_K) return 0;
    const int64_t blocks = (n + RATES_BLOCK - 1) / RATES_BLOCK;
    return lk::align_up((size_t)(blocks > 0 ? blocks : 1) * k * sizeof(double), 256);
}

extern "C" int lk_hpf_rates(const float *d_shp, int64_t n, int32_t k, int32_t ld,
                            double shp_hyper, double prior_ratio, float *d_hyper_rte,
                            const float *d_other_colsum, float *d_rte, float *d_mean,
                            float *d_colsum, void *d_ws, void *stream)
{
    using namespace lk::hpf;
    if (int rc = check_panel("lk_hpf_rates", k, ld)) return rc;
    LK_REQUIRE(n >= 0, "lk_hpf_rates: bad shape");
    LK_REQUIRE(shp_hyper > 0.0 && prior_ratio > 0.0,
               "lk_hpf_rates: the hyper-shape and the prior ratio must be positive");
    LK_REQUIRE(d_other_colsum && d_colsum && d_ws &&
               (n == 0 || (d_shp && d_hyper_rte && d_rte && d_mean)), "lk_hpf_rates: null pointer");
    LK_REQUIRE(((uintptr_t)d_shp | (uintptr_t)d_rte | (uintptr_t)d_mean) % 16 == 0 &&
               (uintptr_t)d_ws % 8 == 0, "lk_hpf_rates: the panels must be 16-byte aligned");
    LK_REQUIRE(d_colsum != d_other_colsum, "lk_hpf_rates: the two column sums must not alias");
    const int64_t blocks = (n + RATES_BLOCK - 1) / RATES_BLOCK;
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_hpf_rates: too many rows");
    hipStream_t st = lk::as_stream(stream);
    if (blocks > 0)
        hipLaunchKernelGGL(rates_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, d_shp, n,
                           (int)k, (int)ld, (float)shp_hyper, prior_ratio, d_hyper_rte,
                           d_other_colsum, d_rte, d_mean, (double *)d_ws);
    hipLaunchKernelGGL(rates_colsum_kernel, dim3(1), dim3(THREADS), 0, st, (const double *)d_ws,
                       blocks, (int)k, d_colsum);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_hpf_loglik_rows(const void *d_indptr, int indptr_is_64,
                                  const int32_t *d_indices, const float *d_values, int64_t n_rows,
                                  int64_t n_cols, int64_t nnz, const float *d_theta,
                                  const float *d_beta, int32_t k, int32_t ld, double *d_out,
                                  void *stream)
{
    using namespace lk::hpf;
    if (int rc = check_panel("lk_hpf_loglik_rows", k, ld)) return rc;
    LK_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "lk_hpf_loglik_rows: bad shape");
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_theta && d_out && (n_cols == 0 || d_beta) &&
               (nnz == 0 || (d_indices && d_values)), "lk_hpf_loglik_rows: null pointer");
    LK_REQUIRE(((uintptr_t)d_theta | (uintptr_t)d_beta) % 16 == 0,
               "lk_hpf_loglik_rows: the panels must be 16-byte aligned");
    const int G = group_lanes(ld);
    const int64_t blocks = (n_rows + THREADS / G - 1) / (THREADS / G);
    LK_REQUIRE(blocks < ((int64_t)1 << 31), "lk_hpf_loglik_rows: too many rows");
    const dim3 grid((unsigned)blocks), blk(THREADS);
    hipStream_t st = lk::as_stream(stream);
#define LK_HPF2(IS64, G_)                                                                        \
    hipLaunchKernelGGL((loglik_rows_kernel<IS64, G_>), grid, blk, 0, st,                         \
                       (const lk::IndPtr<IS64>::type *)d_indptr, d_indices, d_values, n_rows,    \
                       n_cols, nnz, d_theta, d_beta, (int)k, (int)ld, d_out)
#define LK_HPF(G_)                                                                               \
    do {                                                                                         \
        if (indptr_is_64) LK_HPF2(true, G_);                                                     \
        else LK_HPF2(false, G_);                                                                 \
    } while (0)
    if (G == 4) LK_HPF(4);
    else if (G == 8) LK_HPF(8);
    else if (G == 16) LK_HPF(16);
    else if (G == 32) LK_HPF(32);
    else LK_HPF(64);
#undef LK_HPF
#undef LK_HPF2
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
