// spd_blocked.hip -- the inverse of a large dense SPD matrix on gfx950 (EASE's one O(n^3) step,
// `EASEScorer.train`, src/lenskit/knn/ease.py:190-208), and the float32 GEMM it is made of.
//
// lk_gemm_f32: C <- beta C + alpha op(A) op(B), row-major float32, any leading dimensions (int64,
// 4-byte alignment only), any m, n, k >= 0, op = identity or transpose per operand.  A workgroup of
// four waves owns a GT x GT = 128 x 128 tile of C, a wave 64 x 64 of it (2 x 2 accumulators of
// v_mfma_f32_32x32x2_f32).  The operands travel as in topk.hip's score_panel_kernel: the next GK
// = 16 values of k of both panels are fetched into registers while the MFMAs of the current slab
// run out of LDS, where both panels lie k-contiguous with an odd pitch (GK + 1: the 32 rows of an
// operand fetch fall into 32 banks).  The fetch is a guarded scalar load per element -- nothing
// is promised about alignment, edge tiles read zeros -- laid out so that a wave walks along
// whichever index is contiguous in memory for that op.
//   A cell's sum is the k-ordered fmaf chain of the MFMA from zero, then ONE rounding for
// fmaf(alpha, sum, beta * c) (alpha * sum when beta == 0: C is then never read).  No atomics, no
// split-k: the bits of a result depend on its operands alone.
//   The tile mask makes the triangular cases cheap (tile = GT, counted from C's origin):
// LK_GEMM_LOWER computes only the tiles on or below C's diagonal, the others are left untouched;
// LK_GEMM_K_FROM_COL starts a tile's k at its first column (op(B) lower triangular: its rows
// above the tile hold nothing), LK_GEMM_K_FROM_ROW at its first row (op(A) upper triangular).
//
// lk_spd_inverse_blocked: A^-1 in place by a blocked Cholesky, block size NB = GT = 128, every
// step a kernel launch on the caller's stream, no host synchronisation, no waiting kernel:
//   (a) right-looking factorisation A = L L^T.  Block j: lk_chol_upper_inverse on the diagonal
//       block gives L_jj^-1 (float64 sums, rounded once; step = j + 1 for the flag), the panel
//       P = A[>j, j] L_jj^-T is a GEMM into the workspace matrix W (which so collects L's
//       off-diagonal blocks), the trailing update A[>j, >j] -= P P^T covers the lower tiles only;
//   (b) X = L^-1, block row by block row, into A's lower triangle: X[i, i] = L_ii^-1,
//       X[i, <i] = -L_ii^-1 (L[i, <i] X[<i, <i]), the zero tiles of X skipped (K_FROM_COL);
//   (c) A^-1 = X^T X, lower tiles only, k from the tile's first row (LOWER | K_FROM_ROW) into W,
//       then mirrored into both triangles of A: the result is exactly symmetric.
// Not positive definite: lk_chol_upper_inverse replaces the pivot and records block + 1 in *d_flag
// (the first failing block is kept); the steps run on with finite values and the mirror writes
// zeros instead of the result when the flag is set.
#include "common.h"

namespace lk {
namespace spdb {

constexpr int GT = 128;       // tile of C = the block size of the factorisation
constexpr int GK = 16;        // values of k staged per pass
constexpr int GLD = GK + 1;   // conflict-free ds_read_b32 operand fetches
constexpr int64_t MAX_N = (int64_t)1 << 20;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// TA: op(A) = A^T (A is [k x m]); TB: op(B) = B^T (B is [n x k])
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_f32_kernel(
    int64_t m, int64_t n, int64_t k, float alpha, const float *__restrict__ a, int64_t lda,
    const float *__restrict__ b, int64_t ldb, float beta, float *c, int64_t ldc, int mask,
    int64_t n_ctiles)
{
    __shared__ float la[GT * GLD];  // op(A)[i][k]: row i, k contiguous
    __shared__ float lb[GT * GLD];  // op(B)[k][j]: row j, k contiguous
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tr = (int64_t)blockIdx.x / n_ctiles, tc = (int64_t)blockIdx.x % n_ctiles;
    if ((mask & LK_GEMM_LOWER) && tr < tc) return;
    const int64_t i0 = tr * GT, j0 = tc * GT;
    int64_t k0 = 0;
    if ((mask & LK_GEMM_K_FROM_COL) && j0 > k0) k0 = j0;
    if ((mask & LK_GEMM_K_FROM_ROW) && i0 > k0) k0 = i0;
    const int wu = (wave & 1) * 64, wi = (wave >> 1) * 64;

    f32x16 acc[2][2];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ut][t][r] = 0.f;

    constexpr int EV = GT * GK / 256;  // elements per thread and panel
    float ra[EV], rb[EV];
    // element e of a slab -> (row of the tile, k of the slab): a wave's lanes run along the index
    // that is contiguous in memory (rows if the panel is stored k-major, k otherwise)
    auto fetch = [&](int64_t kc) {
#pragma unroll
        for (int q = 0; q < EV; ++q) {
            const int e = tid + q * 256;
            const int r = TA ? e % GT : e / GK, cc = TA ? e / GT : e % GK;
            const int64_t gi = i0 + r, gk = kc + cc;
            ra[q] = 0.f;
            if (gi < m && gk < k) ra[q] = TA ? a[gk * lda + gi] : a[gi * lda + gk];
        }
#pragma unroll
        for (int q = 0; q < EV; ++q) {
            const int e = tid + q * 256;
            const int r = TB ? e / GK : e % GT, cc = TB ? e % GK : e / GT;
            const int64_t gj = j0 + r, gk = kc + cc;
            rb[q] = 0.f;
            if (gj < n && gk < k) rb[q] = TB ? b[gj * ldb + gk] : b[gk * ldb + gj];
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < EV; ++q) {
            const int e = tid + q * 256;
            la[(TA ? e % GT : e / GK) * GLD + (TA ? e / GT : e % GK)] = ra[q];
            lb[(TB ? e / GK : e % GT) * GLD + (TB ? e % GK : e / GT)] = rb[q];
        }
    };

    if (k0 < k) fetch(k0);
    for (int64_t kc = k0; kc < k; kc += GK) {
        stage();
        __syncthreads();
        if (kc + GK < k) fetch(kc + GK);
        // v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int ut = 0; ut < 2; ++ut) av[ut] = la[(wu + ut * 32 + r) * GLD + kk + h];
#pragma unroll
            for (int t = 0; t < 2; ++t) bv[t] = lb[(wi + t * 32 + r) * GLD + kk + h];
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    acc[ut][t] =
                        __builtin_amdgcn_mfma_f32_32x32x2f32(av[ut], bv[t], acc[ut][t], 0, 0, 0);
        }
        __syncthreads();  // everyone is done reading before the next slab is staged
    }

    // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t col = j0 + wi + t * 32 + (lane & 31);
            if (col >= n) continue;
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                const int64_t row = i0 + wu + ut * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);
                if (row >= m) continue;
                float *p = c + row * ldc + col;
                const float s = acc[ut][t][rg];
                *p = beta == 0.f ? alpha * s : __builtin_fmaf(alpha, s, beta * *p);
            }
        }
}

// dst[rows x cols] <- src
__global__ __launch_bounds__(256) void copy_block_kernel(const float *__restrict__ src, int64_t lds,
                                                         float *__restrict__ dst, int64_t ldd,
                                                         int rows, int cols)
{
    for (int p = blockIdx.x * 256 + threadIdx.x; p < rows * cols; p += gridDim.x * 256) {
        const int i = p / cols, j = p % cols;
        dst[(int64_t)i * ldd + j] = src[(int64_t)i * lds + j];
    }
}

// a[i][j] = a[j][i] = w[max(i, j)][min(i, j)] (zeros if the factorisation failed): a 32 x 32 tile
// of the lower triangle per workgroup, transposed through LDS so that both writes are coalesced
__global__ __launch_bounds__(256) void mirror_kernel(const float *__restrict__ w, int64_t ldw,
                                                     float *__restrict__ a, int64_t lda, int64_t n,
                                                     int64_t n_tiles,
                                                     const int32_t *__restrict__ flag)
{
    __shared__ float t[32][33];
    const int64_t tr = (int64_t)blockIdx.x / n_tiles, tc = (int64_t)blockIdx.x % n_tiles;
    if (tr < tc) return;
    const bool bad = *flag != 0;
    const int x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    for (int y = y0; y < 32; y += 8) {
        const int64_t i = tr * 32 + y, j = tc * 32 + x;
        float v = 0.f;
        if (i < n && j < n && !bad) v = i >= j ? w[i * ldw + j] : w[j * ldw + i];
        t[y][x] = v;
        if (i < n && j < n) a[i * lda + j] = v;
    }
    if (tr == tc) return;  // (a diagonal tile is its own mirror image, written above)
    __syncthreads();
    for (int y = y0; y < 32; y += 8) {
        const int64_t i = tc * 32 + y, j = tr * 32 + x;  // the cell (j, i) of the lower tile
        if (i < n && j < n) a[i * lda + j] = t[x][y];
    }
}

static int gemm(int ta, int tb, int64_t m, int64_t n, int64_t k, float alpha, const float *a,
                int64_t lda, const float *b, int64_t ldb, float beta, float *c, int64_t ldc,
                int mask, hipStream_t st)
{
    if (m == 0 || n == 0) return LK_OK;
    const int64_t tiles_r = (m + GT - 1) / GT, tiles_c = (n + GT - 1) / GT;
    LK_REQUIRE(tiles_r * tiles_c < ((int64_t)1 << 31), "lk_gemm_f32: too many tiles");
    const dim3 grid((unsigned)(tiles_r * tiles_c)), blk(256);
#define LK_GEMM_LAUNCH(TA, TB)                                                                   \
    hipLaunchKernelGGL((gemm_f32_kernel<TA, TB>), grid, blk, 0, st, m, n, k, alpha, a, lda, b,   \
                       ldb, beta, c, ldc, mask, tiles_c)
    if (ta && tb) LK_GEMM_LAUNCH(true, true);
    else if (ta) LK_GEMM_LAUNCH(true, false);
    else if (tb) LK_GEMM_LAUNCH(false, true);
    else LK_GEMM_LAUNCH(false, false);
#undef LK_GEMM_LAUNCH
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// the workspace: W [n x n], the diagonal blocks' inverses [blocks x NB x NB], a row panel [NB x n]
struct Ws {
    size_t off_w, off_dinv, off_t, total;
    explicit Ws(int64_t n)
    {
        const size_t blocks = (size_t)((n + GT - 1) / GT);
        off_w = 0;
        off_dinv = align_up((size_t)n * n * sizeof(float), 256);
        off_t = off_dinv + blocks * GT * GT * sizeof(float);
        total = off_t + align_up((size_t)GT * n * sizeof(float), 256);
    }
};

}  // namespace spdb
}  // namespace lk

extern "C" int32_t lk_gemm_tile(void) { return lk::spdb::GT; }

extern "C" int lk_gemm_f32(int trans_a, int trans_b, int64_t m, int64_t n, int64_t k, float alpha,
                           const float *d_a, int64_t lda, const float *d_b, int64_t ldb,
                           float beta, float *d_c, int64_t ldc, int tile_mask, void *stream)
{
    LK_REQUIRE(m >= 0 && n >= 0 && k >= 0, "lk_gemm_f32: bad shape");
    LK_REQUIRE((tile_mask & ~(LK_GEMM_LOWER | LK_GEMM_K_FROM_COL | LK_GEMM_K_FROM_ROW)) == 0,
               "lk_gemm_f32: unknown tile mask bits %d", tile_mask);
    LK_REQUIRE(lda >= (trans_a ? m : k) && ldb >= (trans_b ? k : n) && ldc >= n,
               "lk_gemm_f32: a leading dimension is below the row length");
    if (m == 0 || n == 0) return LK_OK;
    LK_REQUIRE(d_c && (k == 0 || (d_a && d_b)), "lk_gemm_f32: null pointer");
    return lk::spdb::gemm(trans_a != 0, trans_b != 0, m, n, k, alpha, d_a, lda, d_b, ldb, beta,
                          d_c, ldc, tile_mask, lk::as_stream(stream));
}

extern "C" int64_t lk_spd_inverse_blocked_max_n(void) { return lk::spdb::MAX_N; }

extern "C" size_t lk_spd_inverse_blocked_workspace_bytes(int64_t n)
{
    if (n < 1 || n > lk::spdb::MAX_N) return 0;
    return lk::spdb::Ws(n).total;
}

// `phases`: bit 0 = (a), bit 1 = (b), bit 2 = (c) -- the steps of one inversion, queued by one
// call or, for the timing tool, by three on the same matrix and workspace
extern "C" int lk_spd_inverse_blocked_phases(float *d_a, int64_t n, int64_t ld, void *d_work,
                                             size_t work_bytes, int32_t *d_flag, int phases,
                                             void *stream)
{
    using namespace lk;
    using namespace lk::spdb;
    LK_REQUIRE(phases >= 1 && phases <= 7, "lk_spd_inverse_blocked: phases %d outside 1..7",
               phases);
    LK_REQUIRE(n >= 0 && n <= MAX_N, "lk_spd_inverse_blocked: n = %lld outside 0..%lld",
               (long long)n, (long long)MAX_N);
    LK_REQUIRE(ld >= n && ld < ((int64_t)1 << 31), "lk_spd_inverse_blocked: bad leading dimension");
    LK_REQUIRE(d_flag, "lk_spd_inverse_blocked: null flag");
    hipStream_t st = as_stream(stream);
    if (phases & 1) LK_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int32_t), st));
    if (n == 0) return LK_OK;
    const Ws ws(n);
    LK_REQUIRE(d_a && d_work, "lk_spd_inverse_blocked: null pointer");
    LK_REQUIRE(work_bytes >= ws.total, "lk_spd_inverse_blocked: workspace of %zu bytes, %zu needed",
               work_bytes, ws.total);
    LK_REQUIRE((uintptr_t)d_work % 4 == 0 && (uintptr_t)d_a % 4 == 0,
               "lk_spd_inverse_blocked: unaligned pointer");
    char *base = static_cast<char *>(d_work);
    float *w = reinterpret_cast<float *>(base + ws.off_w);
    float *dinv = reinterpret_cast<float *>(base + ws.off_dinv);
    float *tp = reinterpret_cast<float *>(base + ws.off_t);
    const int64_t ldw = n, blocks = (n + GT - 1) / GT;
    int rc;
#define LK_STEP(call)                   \
    do {                                \
        rc = (call);                    \
        if (rc != LK_OK) return rc;     \
    } while (0)

    // (a) A = L L^T: L's off-diagonal blocks into W, the diagonal blocks' inverses into dinv
    for (int64_t j = 0; (phases & 1) && j < blocks; ++j) {
        const int64_t r0 = j * GT;
        const int l = (int)(n - r0 < GT ? n - r0 : GT);
        float *dj = dinv + j * GT * GT;  // [l x l], ld l
        LK_STEP(lk_chol_upper_inverse(d_a + r0 * ld + r0, (int32_t)ld, l, nullptr, dj, l, d_flag,
                                      (int32_t)(j + 1), stream));
        const int64_t rest = n - r0 - l;
        if (rest == 0) break;
        float *p = w + (r0 + l) * ldw + r0;
        LK_STEP(gemm(0, 1, rest, l, l, 1.f, d_a + (r0 + l) * ld + r0, ld, dj, l, 0.f, p, ldw, 0,
                     st));
        LK_STEP(gemm(0, 1, rest, rest, l, -1.f, p, ldw, p, ldw, 1.f,
                     d_a + (r0 + l) * ld + (r0 + l), ld, LK_GEMM_LOWER, st));
    }
    // (b) X = L^-1 into A's lower triangle (the diagonal blocks whole: zeros above the diagonal)
    for (int64_t i = 0; (phases & 2) && i < blocks; ++i) {
        const int64_t r0 = i * GT;
        const int l = (int)(n - r0 < GT ? n - r0 : GT);
        const float *di = dinv + i * GT * GT;
        hipLaunchKernelGGL(copy_block_kernel, dim3((unsigned)((l * l + 255) / 256)), dim3(256), 0,
                           st, di, (int64_t)l, d_a + r0 * ld + r0, ld, l, l);
        if (i == 0) continue;
        LK_STEP(gemm(0, 0, l, r0, r0, 1.f, w + r0 * ldw, ldw, d_a, ld, 0.f, tp, n,
                     LK_GEMM_K_FROM_COL, st));
        LK_STEP(gemm(0, 0, l, r0, l, -1.f, di, l, tp, n, 0.f, d_a + r0 * ld, ld, 0, st));
    }
    LK_HIP_CHECK(hipGetLastError());
    if (!(phases & 4)) return LK_OK;
    // (c) A^-1 = X^T X: lower tiles into W, mirrored into A
    LK_STEP(gemm(1, 0, n, n, n, 1.f, d_a, ld, d_a, ld, 0.f, w, ldw,
                 LK_GEMM_LOWER | LK_GEMM_K_FROM_ROW, st));
#undef LK_STEP
    const int64_t mt = (n + 31) / 32;
    LK_REQUIRE(mt * mt < ((int64_t)1 << 31), "lk_spd_inverse_blocked: too many tiles");
    hipLaunchKernelGGL(mirror_kernel, dim3((unsigned)(mt * mt)), dim3(256), 0, st, w, ldw, d_a, ld,
                       n, mt, d_flag);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_spd_inverse_blocked(float *d_a, int64_t n, int64_t ld, void *d_work,
                                      size_t work_bytes, int32_t *d_flag, void *stream)
{
    return lk_spd_inverse_blocked_phases(d_a, n, ld, d_work, work_bytes, d_flag, 7, stream);
}
