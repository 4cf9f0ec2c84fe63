// lightgcn.hip -- the training step of LightGCN (`lenskit.graphs.lightgcn.LightGCNScorer`) on
// gfx950.
//
// The reference hands the model to an external graph library; its arithmetic is stated in the
// reference tree by `FlexMFModel.update_convolution` / `forward` (src/lenskit/flexmf/_model.py:
// 122-198): the symmetric-normalised propagation  xbar = sum_l alpha_l Mhat^l X  over the bipartite
// interaction graph, differentiated through every batch.  Mhat = diag(d) M diag(d) is symmetric,
// so the backward pass is the forward operator applied to the loss gradient.  Both passes run in
// Horner form, t_j = alpha_j x + Mhat t_{j+1}: one launch of lgcn_propagate_kernel per layer and
// one running panel.  A step is:
//
//   1. L x lgcn_propagate_kernel   X -> xbar;
//   2. lgcn_pair_forward_kernel    one wave per sample: the three scores' rows, the loss term and
//                                  the two loss-gradient coefficients (per-sample scalars);
//      one stable radix sort       (destination node, 3 sample + role) by node (radix_sort.h);
//      lgcn_pair_rowsum_kernel     one wave per touched node walks its entries in sample order
//                                  and accumulates (in float64) coefficient x the other row of
//                                  xbar into the zeroed dense panel g: a store-and-sum scatter,
//                                  no float atomics, one fixed order;
//      flexmf_loss_kernel          the batch loss, summed in sample order by one workgroup;
//   3. L x lgcn_propagate_kernel   g -> dL/dX;
//   4. adamw_dense_kernel          one streaming pass over X and its two moment panels.
//
// lgcn_propagate_kernel has the lane mapping and the arithmetic contract of csr_spmm_kernel
// (svd.hip): a group of G lanes owns a row, a lane one float4 chunk of the panel's row (k <= 256:
// at most 64 chunks, so one chunk per lane); a row of at most SPLIT entries is one
// fused-multiply-add chain per column in entry order; a longer one is cut into segments of SPLIT
// entries that the groups of the workgroup share through LDS and that are added in segment order.
// What differs: no values array -- the weight of an entry is d[column], gathered by the lane that
// loads the index -- the row's own scale b d[r] applied once, after the chain, and the a x[r] term
// fused into the store.
//
// Traffic per propagate pass: nnz (4 ld + 8) bytes gathered (the panel row, the index, d; the
// panel is served from L2 / Infinity Cache) + 8 n ld bytes streamed (x read, out written).
#include "common.h"
#include "flexmf_shared.h"
#include "radix_sort.h"

namespace lk {
namespace lgcn {

constexpr int SPLIT = 256;    // entries per chain segment: lk_spmm_split()
constexpr int THREADS = 256;  // 4 waves
constexpr int UNROLL = 4;
constexpr int WPB = 4;        // waves (samples / nodes) per workgroup of the pair kernels

// the lane's chunk of row c of the panel; an index that is no row of it loads nothing
__device__ __forceinline__ f32x4 load_chunk(const float *__restrict__ t, int ld_t, int64_t n,
                                            bool mine, int j, int32_t c)
{
    f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
    if (mine && c >= 0 && c < n) v = *reinterpret_cast<const f32x4 *>(t + (int64_t)c * ld_t + 4 * j);
    return v;
}

// one chain over the entries [beg, end) of a row, for the lane's chunk: sum d[c] t[c]
template <int G>
__device__ __forceinline__ f32x4 chain(const int32_t *__restrict__ idx,
                                       const float *__restrict__ d, int64_t beg, int64_t end,
                                       const float *__restrict__ t, int ld_t, int64_t n, bool mine,
                                       int j)
{
    f32x4 acc{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t e0 = beg; e0 < end; e0 += G) {
        int32_t ci = -1;
        float wi = 0.0f;
        if (e0 + j < end) {
            ci = idx[e0 + j];
            if (ci >= 0 && ci < n) wi = d[ci];
            else ci = -1;  // an index that is no node: the link is skipped
        }
        const int cnt = end - e0 < G ? (int)(end - e0) : G;
        // the lanes of a group run these loops together: the shuffles stay inside the group.
        // Four entries at a time: their panel rows are requested before the first is used.
        int s = 0;
        for (; s + UNROLL <= cnt; s += UNROLL) {
            int32_t c[UNROLL];
            float w[UNROLL];
            f32x4 tv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                c[u] = __shfl(ci, s + u, G);
                w[u] = __shfl(wi, s + u, G);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) tv[u] = load_chunk(t, ld_t, n, mine, j, c[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (c[u] >= 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = fmaf(w[u], tv[u][q], acc[q]);
                }
        }
        for (; s < cnt; ++s) {
            const int32_t c = __shfl(ci, s, G);
            const float w = __shfl(wi, s, G);
            const f32x4 tv = load_chunk(t, ld_t, n, mine, j, c);
            if (c >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(w, tv[q], acc[q]);
            }
        }
    }
    return acc;
}

// out[r] = a x[r] + (b d[r]) sum_e d[col_e] t[col_e]; x == nullptr: no a x term
template <int G>
__global__ __launch_bounds__(THREADS) void lgcn_propagate_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ idx,
    const float *__restrict__ d, int64_t n, int64_t nnz, float a, const float *__restrict__ x,
    int ld_x, float b, const float *__restrict__ t, int ld_t, int k, float *__restrict__ out,
    int ld_out)
{
    constexpr int NG = THREADS / G;  // rows (groups) per workgroup
    constexpr int W = 4 * G;         // columns a group covers (>= ld_out)
    __shared__ float part[NG * W];   // the segment sums of one round of a long row
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const int chunks_in = (k + 3) / 4, chunks_out = ld_out / 4;
    const bool mine = j < chunks_in;
    const int64_t row0 = (int64_t)blockIdx.x * NG;

    // the extent of a row; offsets that do not describe entries of this matrix make it empty
    auto extent = [&](int64_t r, int64_t &beg, int64_t &end) {
        beg = end = 0;
        if (r < n) {
            const int64_t lo = indptr[r], hi = indptr[r + 1];
            if (lo >= 0 && lo <= hi && hi <= nnz) {
                beg = lo;
                end = hi;
            }
        }
    };
    // one column of the result: the row's scale once, after the chain, then the a x term (xv: the
    // row's x in that column); a row without entries is a x itself
    auto finish = [&](int col, float scale, float sum, float xv, bool empty) -> float {
        if (col >= k) return 0.0f;  // pad columns: zero
        if (empty) return x ? a * xv : 0.0f;
        const float s = scale * sum;
        return x ? fmaf(a, xv, s) : s;
    };

    // rows of at most one segment: one group each
    {
        const int64_t r = row0 + g;
        int64_t beg, end;
        extent(r, beg, end);
        if (r < n && end - beg <= SPLIT) {
            const f32x4 acc = chain<G>(idx, d, beg, end, t, ld_t, n, mine, j);
            if (j < chunks_out) {
                f32x4 o, xv{0.0f, 0.0f, 0.0f, 0.0f};
                if (x && mine) xv = *reinterpret_cast<const f32x4 *>(x + r * ld_x + 4 * j);
                const float scale = b * d[r];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    o[q] = finish(4 * j + q, scale, acc[q], xv[q], end == beg);
                *reinterpret_cast<f32x4 *>(out + r * ld_out + 4 * j) = o;
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
        float tot = 0.0f;  // column threadIdx.x (W <= THREADS)
        for (int64_t s0 = 0; s0 < segs; s0 += NG) {
            const int64_t s = s0 + g;
            if (s < segs) {
                const int64_t sb = beg + s * SPLIT;
                const int64_t se = sb + SPLIT < end ? sb + SPLIT : end;
                const f32x4 acc = chain<G>(idx, d, sb, se, t, ld_t, n, mine, j);
                *reinterpret_cast<f32x4 *>(&part[g * W + 4 * j]) = acc;
            }
            __syncthreads();
            const int live = segs - s0 < NG ? (int)(segs - s0) : NG;
            if (threadIdx.x < W)
                for (int gg = 0; gg < live; ++gg) tot += part[gg * W + threadIdx.x];  // in order
            __syncthreads();
        }
        if ((int)threadIdx.x < ld_out) {
            const int64_t r = row0 + lr;
            const int col = threadIdx.x;
            const float xv = x && col < k ? x[r * ld_x + col] : 0.0f;
            out[r * ld_out + col] = finish(col, b * d[r], tot, xv, false);
        }
    }
}

// ---- pair gradient ---------------------------------------------------------------------------
struct PairScratch {
    float *coef;                // [2 B] dL/ds+ and dL/ds- of the sample
    float *lossv;               // [B] the sample's share of the batch loss
    uint32_t *key[3], *val[3];  // [3 B] in, out, tmp: destination node, 3 sample + role
    void *sort_tmp;
};

static size_t layout(char *base, int64_t B, PairScratch *W)
{
    size_t off = 0;
    PairScratch w{};
    fx::carve(base, off, (size_t)B * 8, (void **)&w.coef);
    fx::carve(base, off, (size_t)B * 4, (void **)&w.lossv);
    for (int i = 0; i < 3; ++i) {
        fx::carve(base, off, (size_t)B * 12, (void **)&w.key[i]);
        fx::carve(base, off, (size_t)B * 12, (void **)&w.val[i]);
    }
    fx::carve(base, off, radix_sort_temp_bytes(3 * B), &w.sort_tmp);
    if (W) *W = w;
    return off;
}

__device__ __forceinline__ bool sample_ok(int32_t u, int32_t ip, int32_t in, int64_t n)
{
    return u >= 0 && u < n && ip >= 0 && ip < n && in >= 0 && in < n;
}

// roles of an entry: 0 the user's row, 1 the positive's, 2 the negative's
template <int KR>
__global__ __launch_bounds__(64 * WPB) void lgcn_pair_forward_kernel(
    const float *__restrict__ xb, int ld, int k, int64_t n, int loss,
    const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
    const int32_t *__restrict__ neg, int64_t B, PairScratch W)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (s >= B) return;
    const int32_t u = users[s], ip = pos[s], in = neg[s];
    const bool ok = sample_ok(u, ip, in, n);  // a sample naming no node takes no part
    float dp = 0.0f, dn = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        if (ok && f < k) {
            const float p = xb[(int64_t)u * ld + f];
            dp += p * xb[(int64_t)ip * ld + f];
            dn += p * xb[(int64_t)in * ld + f];
        }
    }
    const float sp = wave_sum(dp), sn = wave_sum(dn);
    if (lane == 0) {
        const float fB = (float)B;
        float gp, gn, l;
        if (loss == LK_FLEXMF_PAIRWISE) {  // mean -log sigma(s+ - s-)
            const float df = sp - sn;
            gn = fx::sigmoidf(-df) / fB;
            gp = -gn;
            l = fx::softplusf(-df) / fB;
        } else {  // (sum -log sigma(s+) + sum -log sigma(-s-)) / 2B
            const float tot = 2.0f * fB;
            gp = -fx::sigmoidf(-sp) / tot;
            gn = fx::sigmoidf(sn) / tot;
            l = (float)((double)(fx::softplusf(-sp) / tot) + (double)(fx::softplusf(sn) / tot));
        }
        W.coef[2 * s] = ok ? gp : 0.0f;
        W.coef[2 * s + 1] = ok ? gn : 0.0f;
        W.lossv[s] = ok ? l : 0.0f;
        W.key[0][3 * s] = ok ? (uint32_t)u : 0u;
        W.key[0][3 * s + 1] = ok ? (uint32_t)ip : 0u;
        W.key[0][3 * s + 2] = ok ? (uint32_t)in : 0u;
        W.val[0][3 * s] = (uint32_t)(3 * s);
        W.val[0][3 * s + 1] = (uint32_t)(3 * s + 1);
        W.val[0][3 * s + 2] = (uint32_t)(3 * s + 2);
    }
}

// one wave per touched node: its entries in sample order, in float64, rounded once
template <int KR>
__global__ __launch_bounds__(64 * WPB) void lgcn_pair_rowsum_kernel(
    const float *__restrict__ xb, int ld, int k, int64_t n, const int32_t *__restrict__ users,
    const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
    const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval, int64_t E,
    const float *__restrict__ coef, float *__restrict__ g)
{
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (e0 >= E) return;
    const uint32_t row = skey[e0];
    if (e0 > 0 && skey[e0 - 1] == row) return;  // not the head of its node's run
    if (row >= n) return;
    double acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0;
    for (int64_t i = e0; i < E && skey[i] == row; ++i) {
        const uint32_t v = sval[i];
        const int64_t s = v / 3;
        const int role = (int)(v - 3 * s);
        if (!sample_ok(users[s], pos[s], neg[s], n)) continue;
        const double cp = (double)coef[2 * s], cn = (double)coef[2 * s + 1];
        if (role == 0) {  // the user's row: g+ xbar[i+] + g- xbar[i-]
            const float *a = xb + (int64_t)pos[s] * ld, *b = xb + (int64_t)neg[s] * ld;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int f = lane + 64 * r;
                if (f < k) acc[r] += cp * (double)a[f] + cn * (double)b[f];
            }
        } else {  // an item's row: its coefficient times xbar[user]
            const double c = role == 1 ? cp : cn;
            const float *a = xb + (int64_t)users[s] * ld;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int f = lane + 64 * r;
                if (f < k) acc[r] += c * (double)a[f];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        if (f < k) g[(int64_t)row * ld + f] = (float)acc[r];
    }
}

template <int KR>
static int pair_grad_impl(const float *xb, int ld, int k, int64_t n, int loss,
                          const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t B,
                          void *ws, float *g, float *d_loss, float *d_loss_sum, hipStream_t st)
{
    PairScratch W;
    layout(static_cast<char *>(ws), B, &W);
    const int64_t E = 3 * B;
    const dim3 blk(64 * WPB);
    LK_HIP_CHECK(hipMemsetAsync(g, 0, (size_t)n * ld * sizeof(float), st));
    hipLaunchKernelGGL((lgcn_pair_forward_kernel<KR>), dim3((unsigned)((B + WPB - 1) / WPB)), blk,
                       0, st, xb, ld, k, n, loss, users, pos, neg, B, W);
    const int rc = radix_sort_pairs<uint32_t, uint32_t>(W.key[0], W.val[0], W.key[1], W.val[1],
                                                        W.key[2], W.val[2], E, 0, fx::bits_for(n),
                                                        W.sort_tmp, st);
    if (rc != LK_OK) return rc;
    hipLaunchKernelGGL((lgcn_pair_rowsum_kernel<KR>), dim3((unsigned)((E + WPB - 1) / WPB)), blk,
                       0, st, xb, ld, k, n, users, pos, neg, W.key[1], W.val[1], E, W.coef, g);
    hipLaunchKernelGGL(fx::flexmf_loss_kernel, dim3(1), dim3(256), 0, st, W.lossv, B, d_loss,
                       d_loss_sum);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ---- dense AdamW: one streaming pass, a float4 chunk per thread --------------------------------
__global__ __launch_bounds__(256) void adamw_dense_kernel(float *__restrict__ x,
                                                          float *__restrict__ m,
                                                          float *__restrict__ v,
                                                          const float *__restrict__ g,
                                                          int64_t chunks, int chunks_per_row, int k,
                                                          fx::Scalars H)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    const int col0 = 4 * (int)(c % chunks_per_row);
    if (col0 >= k) return;  // a chunk of pad columns: left as it is (zero)
    f32x4 xv = *reinterpret_cast<f32x4 *>(x + 4 * c), mv = *reinterpret_cast<f32x4 *>(m + 4 * c);
    f32x4 vv = *reinterpret_cast<f32x4 *>(v + 4 * c);
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + 4 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (col0 + q < k) {
            float xs = xv[q], ms = mv[q], vs = vv[q];
            fx::adamw(xs, ms, vs, gv[q], H);
            xv[q] = xs;
            mv[q] = ms;
            vv[q] = vs;
        }
    *reinterpret_cast<f32x4 *>(x + 4 * c) = xv;
    *reinterpret_cast<f32x4 *>(m + 4 * c) = mv;
    *reinterpret_cast<f32x4 *>(v + 4 * c) = vv;
}

static int check_panel(const char *who, int64_t n, int32_t k, int32_t ld)
{
    LK_REQUIRE(n >= 1 && n < INT32_MAX, "%s: %lld rows outside 1..2^31-2", who, (long long)n);
    LK_REQUIRE(k >= 1 && k <= LK_FLEXMF_MAX_K, "%s: embedding size %d outside 1..%d", who, k,
               LK_FLEXMF_MAX_K);
    LK_REQUIRE(ld % 4 == 0 && ld >= (k + 3) / 4 * 4 && ld <= LK_FLEXMF_MAX_K,
               "%s: leading dimension %d must be a multiple of 4 in [%d, %d]", who, ld,
               (k + 3) / 4 * 4, LK_FLEXMF_MAX_K);
    return LK_OK;
}

}  // namespace lgcn
}  // namespace lk

extern "C" int lk_lgcn_propagate(const int64_t *d_indptr, const int32_t *d_indices,
                                 const float *d_scale, int64_t n, int64_t nnz, float a,
                                 const float *d_x, float b, const float *d_t, int32_t k, int32_t ld,
                                 float *d_out, void *stream)
{
    using namespace lk::lgcn;
    int rc = check_panel("lk_lgcn_propagate", n, k, ld);
    if (rc != LK_OK) return rc;
    LK_REQUIRE(lk_spmm_split() == SPLIT, "lk_lgcn_propagate: the chain segment differs from "
               "lk_csr_spmm's");
    LK_REQUIRE(nnz >= 0, "lk_lgcn_propagate: bad shape");
    LK_REQUIRE(d_indptr && d_scale && d_t && d_out && (nnz == 0 || d_indices),
               "lk_lgcn_propagate: null pointer");
    LK_REQUIRE(d_out != d_t && d_out != d_x, "lk_lgcn_propagate: the output aliases an input");
    LK_REQUIRE(((uintptr_t)d_x | (uintptr_t)d_t | (uintptr_t)d_out) % 16 == 0,
               "lk_lgcn_propagate: the panels must be 16-byte aligned");
    const int chunks = ld / 4;
    int G = 4;
    while (G < 64 && G < chunks) G *= 2;
    const int64_t blocks = (n + THREADS / G - 1) / (THREADS / G);
    const dim3 grid((unsigned)blocks), blk(THREADS);
    hipStream_t st = lk::as_stream(stream);
#define LK_LGCN_PROP(G_)                                                                        \
    hipLaunchKernelGGL((lgcn_propagate_kernel<G_>), grid, blk, 0, st, d_indptr, d_indices,      \
                       d_scale, n, nnz, a, d_x, (int)ld, b, d_t, (int)ld, (int)k, d_out, (int)ld)
    if (G == 4) LK_LGCN_PROP(4);
    else if (G == 8) LK_LGCN_PROP(8);
    else if (G == 16) LK_LGCN_PROP(16);
    else if (G == 32) LK_LGCN_PROP(32);
    else LK_LGCN_PROP(64);
#undef LK_LGCN_PROP
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" size_t lk_lgcn_pair_grad_workspace_bytes(int64_t batch)
{
    if (batch < 1 || batch >= ((int64_t)1 << 30)) return 0;
    return lk::lgcn::layout(nullptr, batch, nullptr);
}

extern "C" int lk_lgcn_pair_grad(const float *d_xbar, int64_t n, int32_t k, int32_t ld,
                                 int32_t loss, const int32_t *d_users, const int32_t *d_pos,
                                 const int32_t *d_neg, int64_t batch, void *d_ws, float *d_grad,
                                 float *d_loss, float *d_loss_sum, void *stream)
{
    using namespace lk::lgcn;
    int rc = check_panel("lk_lgcn_pair_grad", n, k, ld);
    if (rc != LK_OK) return rc;
    LK_REQUIRE(loss == LK_FLEXMF_LOGISTIC || loss == LK_FLEXMF_PAIRWISE,
               "lk_lgcn_pair_grad: loss %d is neither logistic nor pairwise", loss);
    LK_REQUIRE(batch >= 1 && batch < ((int64_t)1 << 30), "lk_lgcn_pair_grad: bad batch size");
    LK_REQUIRE(d_xbar && d_users && d_pos && d_neg && d_ws && d_grad && d_loss,
               "lk_lgcn_pair_grad: null pointer");
    LK_REQUIRE(d_grad != d_xbar, "lk_lgcn_pair_grad: the gradient aliases the embeddings");
    hipStream_t st = lk::as_stream(stream);
    const int kr = (k + 63) / 64;
    if (kr == 1)
        return pair_grad_impl<1>(d_xbar, ld, k, n, loss, d_users, d_pos, d_neg, batch, d_ws,
                                 d_grad, d_loss, d_loss_sum, st);
    if (kr == 2)
        return pair_grad_impl<2>(d_xbar, ld, k, n, loss, d_users, d_pos, d_neg, batch, d_ws,
                                 d_grad, d_loss, d_loss_sum, st);
    return pair_grad_impl<4>(d_xbar, ld, k, n, loss, d_users, d_pos, d_neg, batch, d_ws, d_grad,
                             d_loss, d_loss_sum, st);
}

extern "C" int lk_adamw_dense(float *d_param, float *d_exp_avg, float *d_exp_avg_sq,
                              const float *d_grad, int64_t n, int32_t k, int32_t ld, double lr,
                              double weight_decay, double beta1, double beta2, double eps,
                              double bias_corr1, double bias_corr2, void *stream)
{
    using namespace lk::lgcn;
    int rc = check_panel("lk_adamw_dense", n, k, ld);
    if (rc != LK_OK) return rc;
    LK_REQUIRE(d_param && d_exp_avg && d_exp_avg_sq && d_grad, "lk_adamw_dense: null pointer");
    LK_REQUIRE(bias_corr1 > 0.0 && bias_corr2 > 0.0, "lk_adamw_dense: bad bias correction");
    LK_REQUIRE(((uintptr_t)d_param | (uintptr_t)d_exp_avg | (uintptr_t)d_exp_avg_sq |
                (uintptr_t)d_grad) % 16 == 0, "lk_adamw_dense: the panels must be 16-byte aligned");
    lk_flexmf_hyper h{};
    h.reg = weight_decay;
    h.lr = lr;
    h.beta1 = beta1;
    h.beta2 = beta2;
    h.eps = eps;
    h.bias_corr1 = bias_corr1;
    h.bias_corr2 = bias_corr2;
    const lk::fx::Scalars H = lk::fx::scalars_of(h);
    const int64_t chunks = n * (ld / 4);
    hipLaunchKernelGGL(adamw_dense_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0,
                       lk::as_stream(stream), d_param, d_exp_avg, d_exp_avg_sq, d_grad, chunks,
                       (int)(ld / 4), (int)k, H);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
