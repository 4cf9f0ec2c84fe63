// flexmf.hip -- the minibatch trainer of FlexMF implicit (logistic, BPR, WARP) on gfx950.
//
// The reference trains this model with a few dozen small Torch launches per batch, samples its
// negatives on the host (src/accel/data/sampling.rs) and crosses to the host inside the WARP
// search (src/lenskit/flexmf/_implicit.py:339-381).  Here a batch is:
//
//   1. flexmf_sample_kernel     one thread per (row, replicate): Philox draw, rejection by a
//                               binary search in the user's sorted CSR row;
//      flexmf_warp_kernel       (misranked negatives) one wave per sample walks its row of a
//                               candidate table, scoring lazily up to the stopping try;
//   2. flexmf_forward_kernel    one wave per sample, a lane per feature: the scores, the loss
//                               term, the loss-gradient COEFFICIENTS and the L2 factors -- per-sample
//                               scalars, no k-wide gradient rows -- and the gathered rows of the
//                               batch staged in scratch (the hazard below);
//   3. two stable radix sorts   (destination row, entry) by row, users and items (radix_sort.h);
//   4. flexmf_rowsum_kernel     one wave per touched row walks its entries in entry order and
//                               accumulates (in float64) coefficient x the other side's STAGED row: a
//                               store-and-sum scatter, no float atomics, one fixed order.
//                               SparseAdam: the update of the row is the kernel's epilogue.
//                               AdamW: the summed gradient goes to scratch and
//      flexmf_adamw_kernel      streams once over every row of every table.
//   5. flexmf_loss_kernel       the batch loss, summed in sample order by one workgroup.
//
// The hazard: within one step the user update reads item rows and the item update reads user
// rows, and both must see the values from before the step -- while a batch may hold the same
// user hundreds of times, and a negative may equal its own positive or another sample's item.
// The forward kernel therefore copies every row it gathers into scratch (batch x (2 + n_neg) rows:
// 6 MB at batch 8192, k 64, one negative) BEFORE anything is written; the row-sum kernels read the
// other side from that copy only, and a row's own old value is read by the one wave that owns it.
//
// FlexMF explicit (lk_flexmf_step_explicit) is the same step without negatives: a rating per
// sample, squared error, and an L2 term whose weights are the same on both sides.  It has a
// forward kernel and a row-sum kernel of its own (flexmf_forward_mse_kernel,
// flexmf_rowsum_mse_kernel) and shares the sorts, the optimiser updates, the AdamW pass, the loss
// kernel and the scratch layout (with no negatives: E = B) with the implicit step, whose kernels
// are as they were.
#include <math.h>

#include "common.h"
#include "flexmf_shared.h"
#include "philox.h"
#include "radix_sort.h"

namespace lk {
namespace fx {

constexpr int WPB = 4;  // waves (samples / rows) per workgroup

struct Scratch {
    float *Ps, *Qs;        // staged rows: [B x k], [E x k]   (E = B (1 + n_neg))
    float *g_item;         // [E] dL/ds of the entry's score
    float *c_item;         // [E] L2 factor of the entry's item row
    float *gsum_user;      // [B] sum of the sample's score gradients (user bias)
    float *c_user;         // [B] L2 factor of the sample's user row
    float *lossv;          // [B] the sample's share of the batch loss
    uint32_t *ukey[3], *uval[3];  // in, out, tmp
    uint32_t *ikey[3], *ival[3];
    void *sort_tmp;
    float *G, *gb;         // AdamW: summed gradients [(B + E) x k], [(B + E)]
};

// ---- negative sampling ---------------------------------------------------------------------
__device__ __forceinline__ bool row_contains(const int32_t *__restrict__ cols, int64_t lo,
                                             int64_t hi, int32_t c)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int32_t v = cols[mid];
        if (v == c) return true;
        if (v < c) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(256) void flexmf_sample_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ cols, int64_t nnz,
    int64_t n_cols, const int32_t *__restrict__ rows, int64_t n_rows, int n, int popular,
    int verify, int max_attempts, uint64_t key, uint64_t counter, int32_t *__restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_rows * n) return;
    const int64_t r = idx / n;
    const uint32_t j = (uint32_t)(idx - r * n);
    const int32_t row = rows[r];
    const int64_t lo = indptr[row], hi = indptr[row + 1];
    const Philox ph{(uint32_t)key, (uint32_t)(key >> 32)};
    int32_t col = 0;
    for (int attempt = 0;; ++attempt) {
        uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)r,
                         (j << 8) | (uint32_t)attempt};
        ph(c);
        const uint64_t u = ((uint64_t)c[1] << 32) | c[0];
        if (popular)
            col = cols[__umul64hi(u, (uint64_t)nnz)];
        else
            col = (int32_t)__umul64hi(u, (uint64_t)n_cols);
        if (!verify || attempt >= max_attempts || !row_contains(cols, lo, hi, col)) break;
    }
    out[idx] = col;
}

__global__ __launch_bounds__(256) void flexmf_gather_kernel(
    const int32_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ all_users,
    const int32_t *__restrict__ all_items, int32_t *__restrict__ users, int32_t *__restrict__ items)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t s = perm[i];
    users[i] = all_users[s];
    items[i] = all_items[s];
}

__global__ __launch_bounds__(256) void flexmf_gather_values_kernel(
    const int32_t *__restrict__ perm, int64_t n, const float *__restrict__ all,
    float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = all[perm[i]];
}

// ---- WARP search ---------------------------------------------------------------------------
template <int KR>
__global__ __launch_bounds__(64 * WPB) void flexmf_warp_kernel(
    lk_flexmf_tables T, const int32_t *__restrict__ users, const int32_t *__restrict__ pos,
    const int32_t *__restrict__ cand, int64_t B, int tries, int32_t *__restrict__ out_neg,
    int32_t *__restrict__ out_count, double *__restrict__ out_weight)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const int k = T.k;
    const int32_t u = users[b], ip = pos[b];
    const float *P = T.param[0], *Q = T.param[1], *ub = T.param[2], *ib = T.param[3];
    float p[KR];
    float dot = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        p[r] = f < k ? P[(int64_t)u * k + f] : 0.0f;
        dot += p[r] * (f < k ? Q[(int64_t)ip * k + f] : 0.0f);
    }
    const float bu = ub ? ub[u] : 0.0f;
    const float sp = (bu + (ib ? ib[ip] : 0.0f)) + wave_sum(dot);
    float best = -INFINITY;
    int32_t best_item = 0, count = 0;
    for (int t = 1; t <= tries; ++t) {
        const int32_t c = cand[b * tries + (t - 1)];
        float d = 0.0f;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int f = lane + 64 * r;
            d += p[r] * (f < k ? Q[(int64_t)c * k + f] : 0.0f);
        }
        const float s = (bu + (ib ? ib[c] : 0.0f)) + wave_sum(d);
        if (s > best) {
            best = s;
            best_item = c;
            count = t;
        }
        if (best >= sp) break;  // wave-uniform: every lane holds the same sums
    }
    if (lane == 0) {
        const double rank = (double)(T.n_items - 1) / ((double)count + 1.0);
        const double r2 = rank * rank;
        out_neg[b] = best_item;
        out_count[b] = count;
        out_weight[b] = log(rank) + 0.57721566490153286061 + 1.0 / (2.0 * rank) -
                        1.0 / (12.0 * r2) + 1.0 / (120.0 * r2 * r2);
    }
}

// ---- forward + loss gradient ---------------------------------------------------------------
template <int KR>
__global__ __launch_bounds__(64 * WPB) void flexmf_forward_kernel(
    lk_flexmf_tables T, Scalars H, const int32_t *__restrict__ users,
    const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
    const double *__restrict__ weights, int64_t B, Scratch W)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const int k = T.k, n = H.n_neg;
    const int32_t u = users[b], ip = pos[b];
    const float *P = T.param[0], *Q = T.param[1], *ub = T.param[2], *ib = T.param[3];
    const float fB = (float)B, fBn = (float)B * (float)n;
    float p[KR];
    float dot = 0.0f, pn = 0.0f, qn = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        const bool ok = f < k;
        p[r] = ok ? P[(int64_t)u * k + f] : 0.0f;
        const float q = ok ? Q[(int64_t)ip * k + f] : 0.0f;
        dot += p[r] * q;
        pn += p[r] * p[r];
        qn += q * q;
        if (ok) {
            W.Ps[b * k + f] = p[r];
            W.Qs[b * k + f] = q;
        }
    }
    const float bu = ub ? ub[u] : 0.0f;
    const float bip = ib ? ib[ip] : 0.0f;
    const float sp = (bu + bip) + wave_sum(dot);
    float pnorm = 0.0f, l2acc = 0.0f, c_user = 0.0f, c_pos = 0.0f;
    if (H.l2) {
        pnorm = sqrtf(wave_sum(pn));
        const float qnorm = sqrtf(wave_sum(qn));
        // d||x||/dx = x / ||x||, and 0 at x = 0 (what Torch returns)
        c_user = pnorm > 0.0f ? H.reg / (fB * pnorm) : 0.0f;
        c_pos = qnorm > 0.0f ? 0.5f * H.reg / (fB * qnorm) : 0.0f;
        l2acc = (bu * bu + bip * bip + pnorm + qnorm) / fB;
    }
    float gpos = 0.0f, gsum = 0.0f;
    double lossacc = 0.0;
    const float ftot = fB + fBn;
    if (H.loss == LK_FLEXMF_LOGISTIC) {
        gpos = -H.pos_weight * sigmoidf(-sp) / ftot;
        lossacc = (double)(H.pos_weight * softplusf(-sp) / ftot);
    }
    for (int j = 0; j < n; ++j) {
        const int64_t e = B + b * n + j;
        const int32_t in = neg[b * n + j];
        float d = 0.0f, nn = 0.0f;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int f = lane + 64 * r;
            const float q = f < k ? Q[(int64_t)in * k + f] : 0.0f;
            d += p[r] * q;
            nn += q * q;
            if (f < k) W.Qs[e * k + f] = q;
        }
        const float bin = ib ? ib[in] : 0.0f;
        const float sn = (bu + bin) + wave_sum(d);
        float gneg;
        if (H.loss == LK_FLEXMF_LOGISTIC) {
            gneg = sigmoidf(sn) / ftot;
            lossacc += (double)(softplusf(sn) / ftot);
        } else if (H.loss == LK_FLEXMF_PAIRWISE) {
            const float df = sp - sn;
            gneg = sigmoidf(-df) / fBn;
            gpos -= gneg;
            lossacc += (double)(softplusf(-df) / fBn);
        } else {  // WARP: the float32 term times the float64 weight, as Torch promotes it
            const float df = sp - sn;
            const double w = weights[b];
            gneg = (float)((double)sigmoidf(-df) * w / (double)B);
            gpos -= gneg;
            lossacc += (double)softplusf(-df) * w / (double)B;
        }
        gsum += gneg;
        float c_neg = 0.0f;
        if (H.l2) {
            const float qnorm = sqrtf(wave_sum(nn));
            c_neg = qnorm > 0.0f ? 0.5f * H.reg / (fBn * qnorm) : 0.0f;
            l2acc += (bu * bu + bin * bin + pnorm + qnorm) / fBn;
        }
        if (lane == 0) {
            W.g_item[e] = gneg;
            W.c_item[e] = c_neg;
            W.ikey[0][e] = (uint32_t)in;
            W.ival[0][e] = (uint32_t)e;
        }
    }
    gsum += gpos;
    if (lane == 0) {
        W.g_item[b] = gpos;
        W.c_item[b] = c_pos;
        W.ikey[0][b] = (uint32_t)ip;
        W.ival[0][b] = (uint32_t)b;
        W.ukey[0][b] = (uint32_t)u;
        W.uval[0][b] = (uint32_t)b;
        W.gsum_user[b] = gsum;
        W.c_user[b] = c_user;
        W.lossv[b] = (float)(lossacc + (double)(H.reg * 0.5f * l2acc) * (H.l2 ? 1.0 : 0.0));
    }
}

// ---- per-destination sum (+ SparseAdam) ------------------------------------------------------
__device__ __forceinline__ void sparse_adam(float &x, float &m, float &v, float g, const Scalars &H)
{
    // torch.optim._functional.sparse_adam on the coalesced gradient
    m = m + (g - m) * H.omb1;
    v = v + (g * g - v) * H.omb2;
    x = x + (-H.sparse_step) * (m / (sqrtf(v) + H.eps));
}

template <int KR, bool ITEM, bool FUSED>
__global__ __launch_bounds__(64 * WPB) void flexmf_rowsum_kernel(
    lk_flexmf_tables T, Scalars H, const uint32_t *__restrict__ skey,
    const uint32_t *__restrict__ sval, int64_t E, int64_t B, Scratch W, int64_t g_off,
    int32_t *__restrict__ slot)
{
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (e0 >= E) return;
    const uint32_t row = skey[e0];
    if (e0 > 0 && skey[e0 - 1] == row) return;  // not the head of its row's run
    const int k = T.k, n = H.n_neg;
    const float fB = (float)B, fBn = (float)B * (float)n;
    // float64 accumulators: a row's run may be the whole batch (one user 8192 times), and a
    // sequential float32 sum of that many terms is further from the exact sum than Torch's own
    // float32 reduction; the sum is rounded to float32 once, at the end
    double acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0;
    double gb = 0.0, cself = 0.0, cbias = 0.0;
    for (int64_t i = e0; i < E && skey[i] == row; ++i) {
        const int64_t s = sval[i];
        if (ITEM) {
            const double coef = (double)W.g_item[s];
            const int64_t b = s < B ? s : (s - B) / n;
            const float *other = W.Ps + b * k;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int f = lane + 64 * r;
                if (f < k) acc[r] += coef * (double)other[f];
            }
            gb += coef;
            cself += (double)W.c_item[s];
            if (H.l2) cbias += (double)(s < B ? H.reg / fB : H.reg / fBn);
        } else {
            for (int j = -1; j < n; ++j) {
                const int64_t e = j < 0 ? s : B + s * n + j;
                const double coef = (double)W.g_item[e];
                const float *other = W.Qs + e * k;
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const int f = lane + 64 * r;
                    if (f < k) acc[r] += coef * (double)other[f];
                }
            }
            gb += (double)W.gsum_user[s];
            cself += (double)W.c_user[s];
            if (H.l2) cbias += (double)(2.0f * H.reg / fB);
        }
    }
    const int ti = ITEM ? 1 : 0, tb = ITEM ? 3 : 2;
    float *X = T.param[ti] + (int64_t)row * k;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        if (f < k) {
            float x = X[f];
            const float g = (float)(acc[r] + cself * (double)x);
            if (FUSED) {
                float *M = T.exp_avg[ti] + (int64_t)row * k, *V = T.exp_avg_sq[ti] + (int64_t)row * k;
                float m = M[f], v = V[f];
                sparse_adam(x, m, v, g, H);
                X[f] = x;
                M[f] = m;
                V[f] = v;
            } else {
                W.G[(g_off + e0) * k + f] = g;
            }
        }
    }
    if (lane == 0) {
        if (T.param[tb]) {
            float x = T.param[tb][row];
            const float g = (float)(gb + cbias * (double)x);
            if (FUSED) {
                float m = T.exp_avg[tb][row], v = T.exp_avg_sq[tb][row];
                sparse_adam(x, m, v, g, H);
                T.param[tb][row] = x;
                T.exp_avg[tb][row] = m;
                T.exp_avg_sq[tb][row] = v;
            } else {
                W.gb[g_off + e0] = g;
            }
        }
        if (!FUSED) slot[(ITEM ? T.n_users : 0) + row] = (int32_t)(g_off + e0);
    }
}

// ---- AdamW: one streaming pass over every row of every table ---------------------------------
template <int KR>
__global__ __launch_bounds__(64 * WPB) void flexmf_adamw_kernel(lk_flexmf_tables T, Scalars H,
                                                                Scratch W,
                                                                int32_t *__restrict__ slot)
{
    const int lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (r0 >= T.n_users + T.n_items) return;
    const bool item = r0 >= T.n_users;
    const int64_t row = item ? r0 - T.n_users : r0;
    const int ti = item ? 1 : 0, tb = item ? 3 : 2;
    const int k = T.k;
    const int32_t s = slot[r0];
    float *X = T.param[ti] + row * k, *M = T.exp_avg[ti] + row * k, *V = T.exp_avg_sq[ti] + row * k;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        if (f < k) {
            const float g = s >= 0 ? W.G[(int64_t)s * k + f] : 0.0f;
            float x = X[f], m = M[f], v = V[f];
            adamw(x, m, v, g, H);
            X[f] = x;
            M[f] = m;
            V[f] = v;
        }
    }
    if (lane == 0) {
        if (T.param[tb]) {
            const float g = s >= 0 ? W.gb[s] : 0.0f;
            float x = T.param[tb][row], m = T.exp_avg[tb][row], v = T.exp_avg_sq[tb][row];
            adamw(x, m, v, g, H);
            T.param[tb][row] = x;
            T.exp_avg[tb][row] = m;
            T.exp_avg_sq[tb][row] = v;
        }
        if (s >= 0) slot[r0] = -1;  // left as found: all -1
    }
}

// ---- FlexMF explicit: squared error on (user, item, rating) -----------------------------------
// pred = (b_u + b_i) + p_u . q_i;  loss = mean (pred - r)^2;  dL/dpred = 2 (pred - r) / B.
// reg_method "L2" adds reg * mean(b_u^2 + b_i^2 + |p_u| + |q_i|): per occurrence reg x / (B |x|)
// to an embedding row (0 at x = 0) and 2 reg b / B to a bias, the same on both sides.
template <int KR>
__global__ __launch_bounds__(64 * WPB) void flexmf_forward_mse_kernel(
    lk_flexmf_tables T, Scalars H, const int32_t *__restrict__ users,
    const int32_t *__restrict__ items, const float *__restrict__ ratings, int64_t B, Scratch W)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const int k = T.k;
    const int32_t u = users[b], i = items[b];
    const float *P = T.param[0], *Q = T.param[1], *ub = T.param[2], *ib = T.param[3];
    const float fB = (float)B;
    float dot = 0.0f, pn = 0.0f, qn = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        const bool ok = f < k;
        const float p = ok ? P[(int64_t)u * k + f] : 0.0f;
        const float q = ok ? Q[(int64_t)i * k + f] : 0.0f;
        dot += p * q;
        pn += p * p;
        qn += q * q;
        if (ok) {
            W.Ps[b * k + f] = p;
            W.Qs[b * k + f] = q;
        }
    }
    const float pred = ((ub ? ub[u] : 0.0f) + (ib ? ib[i] : 0.0f)) + wave_sum(dot);
    float c_user = 0.0f, c_item = 0.0f;
    if (H.l2) {
        const float pnorm = sqrtf(wave_sum(pn)), qnorm = sqrtf(wave_sum(qn));
        c_user = pnorm > 0.0f ? H.reg / (fB * pnorm) : 0.0f;
        c_item = qnorm > 0.0f ? H.reg / (fB * qnorm) : 0.0f;
    }
    if (lane == 0) {
        const float diff = pred - ratings[b];
        const float g = 2.0f * diff / fB;
        W.g_item[b] = g;
        W.gsum_user[b] = g;
        W.c_item[b] = c_item;
        W.c_user[b] = c_user;
        W.ikey[0][b] = (uint32_t)i;
        W.ival[0][b] = (uint32_t)b;
        W.ukey[0][b] = (uint32_t)u;
        W.uval[0][b] = (uint32_t)b;
        W.lossv[b] = diff * diff / fB;  // the squared error alone: the L2 term is not reported
    }
}

// one wave per touched row, either side: its samples in sample order, in float64
template <int KR, bool ITEM, bool FUSED>
__global__ __launch_bounds__(64 * WPB) void flexmf_rowsum_mse_kernel(
    lk_flexmf_tables T, Scalars H, const uint32_t *__restrict__ skey,
    const uint32_t *__restrict__ sval, int64_t B, Scratch W, int64_t g_off,
    int32_t *__restrict__ slot)
{
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (e0 >= B) return;
    const uint32_t row = skey[e0];
    if (e0 > 0 && skey[e0 - 1] == row) return;  // not the head of its row's run
    const int k = T.k;
    const float *staged = ITEM ? W.Ps : W.Qs;  // the other side, as it was before the step
    const float *cvec = ITEM ? W.c_item : W.c_user;
    const double cb1 = H.l2 ? (double)(2.0f * H.reg / (float)B) : 0.0;
    double acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0;
    double gb = 0.0, cself = 0.0, cbias = 0.0;
    for (int64_t i = e0; i < B && skey[i] == row; ++i) {
        const int64_t s = sval[i];
        const double coef = (double)W.g_item[s];
        const float *other = staged + s * k;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int f = lane + 64 * r;
            if (f < k) acc[r] += coef * (double)other[f];
        }
        gb += coef;
        cself += (double)cvec[s];
        cbias += cb1;
    }
    const int ti = ITEM ? 1 : 0, tb = ITEM ? 3 : 2;
    float *X = T.param[ti] + (int64_t)row * k;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int f = lane + 64 * r;
        if (f < k) {
            float x = X[f];
            const float g = (float)(acc[r] + cself * (double)x);
            if (FUSED) {
                float *M = T.exp_avg[ti] + (int64_t)row * k, *V = T.exp_avg_sq[ti] + (int64_t)row * k;
                float m = M[f], v = V[f];
                sparse_adam(x, m, v, g, H);
                X[f] = x;
                M[f] = m;
                V[f] = v;
            } else {
                W.G[(g_off + e0) * k + f] = g;
            }
        }
    }
    if (lane == 0) {
        if (T.param[tb]) {
            float x = T.param[tb][row];
            const float g = (float)(gb + cbias * (double)x);
            if (FUSED) {
                float m = T.exp_avg[tb][row], v = T.exp_avg_sq[tb][row];
                sparse_adam(x, m, v, g, H);
                T.param[tb][row] = x;
                T.exp_avg[tb][row] = m;
                T.exp_avg_sq[tb][row] = v;
            } else {
                W.gb[g_off + e0] = g;
            }
        }
        if (!FUSED) slot[(ITEM ? T.n_users : 0) + row] = (int32_t)(g_off + e0);
    }
}

// the scratch layout of a step; base == nullptr: only the size
static size_t layout(char *base, int64_t B, int n, int k, Scratch *W)
{
    const int64_t E = B * (1 + n);
    size_t off = 0;
    Scratch w{};
    carve(base, off, (size_t)B * k * 4, (void **)&w.Ps);
    carve(base, off, (size_t)E * k * 4, (void **)&w.Qs);
    carve(base, off, (size_t)E * 4, (void **)&w.g_item);
    carve(base, off, (size_t)E * 4, (void **)&w.c_item);
    carve(base, off, (size_t)B * 4, (void **)&w.gsum_user);
    carve(base, off, (size_t)B * 4, (void **)&w.c_user);
    carve(base, off, (size_t)B * 4, (void **)&w.lossv);
    for (int i = 0; i < 3; ++i) {
        carve(base, off, (size_t)B * 4, (void **)&w.ukey[i]);
        carve(base, off, (size_t)B * 4, (void **)&w.uval[i]);
        carve(base, off, (size_t)E * 4, (void **)&w.ikey[i]);
        carve(base, off, (size_t)E * 4, (void **)&w.ival[i]);
    }
    carve(base, off, radix_sort_temp_bytes(E), &w.sort_tmp);
    carve(base, off, (size_t)(B + E) * k * 4, (void **)&w.G);
    carve(base, off, (size_t)(B + E) * 4, (void **)&w.gb);
    if (W) *W = w;
    return off;
}

static int check_tables(const lk_flexmf_tables *T, const char *who)
{
    LK_REQUIRE(T, "%s: null tables", who);
    LK_REQUIRE(T->k >= 1 && T->k <= LK_FLEXMF_MAX_K, "%s: embedding size %d outside 1..%d", who,
               T->k, LK_FLEXMF_MAX_K);
    LK_REQUIRE(T->n_users >= 1 && T->n_items >= 1 && T->n_users < INT32_MAX &&
                   T->n_items < INT32_MAX, "%s: bad table shape", who);
    LK_REQUIRE(T->param[0] && T->param[1], "%s: null embedding table", who);
    return LK_OK;
}

template <int KR>
static int step_impl(const lk_flexmf_tables &T, const Scalars &H, bool adamw_opt,
                     const int32_t *users, const int32_t *pos, const int32_t *neg,
                     const double *weights, int64_t B, void *ws, int32_t *slot, float *loss,
                     float *loss_sum, hipStream_t st)
{
    Scratch W;
    layout(static_cast<char *>(ws), B, H.n_neg, T.k, &W);
    const int64_t E = B * (1 + H.n_neg);
    const dim3 blk(64 * WPB);
    hipLaunchKernelGGL((flexmf_forward_kernel<KR>), dim3((unsigned)((B + WPB - 1) / WPB)), blk, 0,
                       st, T, H, users, pos, neg, weights, B, W);
    int rc = radix_sort_pairs<uint32_t, uint32_t>(W.ukey[0], W.uval[0], W.ukey[1], W.uval[1],
                                                  W.ukey[2], W.uval[2], B, 0,
                                                  bits_for(T.n_users), W.sort_tmp, st);
    if (rc != LK_OK) return rc;
    rc = radix_sort_pairs<uint32_t, uint32_t>(W.ikey[0], W.ival[0], W.ikey[1], W.ival[1],
                                              W.ikey[2], W.ival[2], E, 0, bits_for(T.n_items),
                                              W.sort_tmp, st);
    if (rc != LK_OK) return rc;
    const dim3 gu((unsigned)((B + WPB - 1) / WPB)), gi((unsigned)((E + WPB - 1) / WPB));
    if (adamw_opt) {
        hipLaunchKernelGGL((flexmf_rowsum_kernel<KR, false, false>), gu, blk, 0, st, T, H,
                           W.ukey[1], W.uval[1], B, B, W, (int64_t)0, slot);
        hipLaunchKernelGGL((flexmf_rowsum_kernel<KR, true, false>), gi, blk, 0, st, T, H,
                           W.ikey[1], W.ival[1], E, B, W, B, slot);
        const int64_t rows = T.n_users + T.n_items;
        hipLaunchKernelGGL((flexmf_adamw_kernel<KR>), dim3((unsigned)((rows + WPB - 1) / WPB)),
                           blk, 0, st, T, H, W, slot);
    } else {
        hipLaunchKernelGGL((flexmf_rowsum_kernel<KR, false, true>), gu, blk, 0, st, T, H,
                           W.ukey[1], W.uval[1], B, B, W, (int64_t)0, slot);
        hipLaunchKernelGGL((flexmf_rowsum_kernel<KR, true, true>), gi, blk, 0, st, T, H,
                           W.ikey[1], W.ival[1], E, B, W, B, slot);
    }
    hipLaunchKernelGGL(flexmf_loss_kernel, dim3(1), dim3(256), 0, st, W.lossv, B, loss, loss_sum);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

template <int KR>
static int step_mse_impl(const lk_flexmf_tables &T, const Scalars &H, bool adamw_opt,
                         const int32_t *users, const int32_t *items, const float *ratings,
                         int64_t B, void *ws, int32_t *slot, float *loss, float *loss_sum,
                         hipStream_t st)
{
    Scratch W;
    layout(static_cast<char *>(ws), B, 0, T.k, &W);
    const dim3 blk(64 * WPB), grid((unsigned)((B + WPB - 1) / WPB));
    hipLaunchKernelGGL((flexmf_forward_mse_kernel<KR>), grid, blk, 0, st, T, H, users, items,
                       ratings, B, W);
    int rc = radix_sort_pairs<uint32_t, uint32_t>(W.ukey[0], W.uval[0], W.ukey[1], W.uval[1],
                                                  W.ukey[2], W.uval[2], B, 0,
                                                  bits_for(T.n_users), W.sort_tmp, st);
    if (rc != LK_OK) return rc;
    rc = radix_sort_pairs<uint32_t, uint32_t>(W.ikey[0], W.ival[0], W.ikey[1], W.ival[1],
                                              W.ikey[2], W.ival[2], B, 0, bits_for(T.n_items),
                                              W.sort_tmp, st);
    if (rc != LK_OK) return rc;
    if (adamw_opt) {
        hipLaunchKernelGGL((flexmf_rowsum_mse_kernel<KR, false, false>), grid, blk, 0, st, T, H,
                           W.ukey[1], W.uval[1], B, W, (int64_t)0, slot);
        hipLaunchKernelGGL((flexmf_rowsum_mse_kernel<KR, true, false>), grid, blk, 0, st, T, H,
                           W.ikey[1], W.ival[1], B, W, B, slot);
        const int64_t rows = T.n_users + T.n_items;
        hipLaunchKernelGGL((flexmf_adamw_kernel<KR>), dim3((unsigned)((rows + WPB - 1) / WPB)),
                           blk, 0, st, T, H, W, slot);
    } else {
        hipLaunchKernelGGL((flexmf_rowsum_mse_kernel<KR, false, true>), grid, blk, 0, st, T, H,
                           W.ukey[1], W.uval[1], B, W, (int64_t)0, slot);
        hipLaunchKernelGGL((flexmf_rowsum_mse_kernel<KR, true, true>), grid, blk, 0, st, T, H,
                           W.ikey[1], W.ival[1], B, W, B, slot);
    }
    hipLaunchKernelGGL(flexmf_loss_kernel, dim3(1), dim3(256), 0, st, W.lossv, B, loss, loss_sum);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace fx
}  // namespace lk

extern "C" int lk_flexmf_sample_negatives(const int64_t *d_indptr, const int32_t *d_indices,
                                          int64_t nnz, int64_t n_cols, const int32_t *d_rows,
                                          int64_t n_rows, int32_t n, int popular, int verify,
                                          int32_t max_attempts, uint64_t key, uint64_t counter,
                                          int32_t *d_out, void *stream)
{
    LK_REQUIRE(n_rows >= 0 && n >= 1 && n < (1 << 24) && n_cols >= 1 && n_cols < INT32_MAX,
               "lk_flexmf_sample_negatives: bad shape");
    LK_REQUIRE(max_attempts >= 0 && max_attempts < 256,
               "lk_flexmf_sample_negatives: max_attempts outside 0..255");
    LK_REQUIRE(n_rows < ((int64_t)1 << 32), "lk_flexmf_sample_negatives: too many rows");
    LK_REQUIRE(!popular || nnz >= 1, "lk_flexmf_sample_negatives: popular sampling of no entries");
    if (n_rows == 0) return LK_OK;
    LK_REQUIRE(d_indptr && d_indices && d_rows && d_out,
               "lk_flexmf_sample_negatives: null pointer");
    const int64_t total = n_rows * n;
    hipLaunchKernelGGL(lk::fx::flexmf_sample_kernel, dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, lk::as_stream(stream), d_indptr, d_indices, nnz, n_cols,
                       d_rows, n_rows, (int)n, popular, verify, (int)max_attempts, key, counter,
                       d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_flexmf_gather_batch(const int32_t *d_perm, int64_t n,
                                      const int32_t *d_all_users, const int32_t *d_all_items,
                                      int32_t *d_users, int32_t *d_items, void *stream)
{
    LK_REQUIRE(n >= 0, "lk_flexmf_gather_batch: bad length");
    if (n == 0) return LK_OK;
    LK_REQUIRE(d_perm && d_all_users && d_all_items && d_users && d_items,
               "lk_flexmf_gather_batch: null pointer");
    hipLaunchKernelGGL(lk::fx::flexmf_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256),
                       0, lk::as_stream(stream), d_perm, n, d_all_users, d_all_items, d_users,
                       d_items);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_flexmf_warp_search(const lk_flexmf_tables *tables, const int32_t *d_users,
                                     const int32_t *d_pos, const int32_t *d_cand, int64_t batch,
                                     int32_t tries, int32_t *d_neg, int32_t *d_count,
                                     double *d_weight, void *stream)
{
    int rc = lk::fx::check_tables(tables, "lk_flexmf_warp_search");
    if (rc != LK_OK) return rc;
    LK_REQUIRE(batch >= 0 && tries >= 1, "lk_flexmf_warp_search: bad shape");
    if (batch == 0) return LK_OK;
    LK_REQUIRE(d_users && d_pos && d_cand && d_neg && d_count && d_weight,
               "lk_flexmf_warp_search: null pointer");
    const dim3 grid((unsigned)((batch + lk::fx::WPB - 1) / lk::fx::WPB)), blk(64 * lk::fx::WPB);
    hipStream_t st = lk::as_stream(stream);
    const int kr = (tables->k + 63) / 64;
#define LK_FX_WARP(KR)                                                                          \
    hipLaunchKernelGGL((lk::fx::flexmf_warp_kernel<KR>), grid, blk, 0, st, *tables, d_users,     \
                       d_pos, d_cand, batch, (int)tries, d_neg, d_count, d_weight)
    if (kr == 1) LK_FX_WARP(1);
    else if (kr == 2) LK_FX_WARP(2);
    else LK_FX_WARP(4);
#undef LK_FX_WARP
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" size_t lk_flexmf_step_workspace_bytes(int64_t batch, int32_t n_neg, int32_t k)
{
    if (batch < 1 || n_neg < 1 || k < 1 || k > LK_FLEXMF_MAX_K) return 0;
    return lk::fx::layout(nullptr, batch, n_neg, k, nullptr);
}

extern "C" int lk_flexmf_step(const lk_flexmf_tables *tables, const lk_flexmf_hyper *hyper,
                              const int32_t *d_users, const int32_t *d_pos, const int32_t *d_neg,
                              const double *d_weights, int64_t batch, void *d_ws, int32_t *d_slot,
                              float *d_loss, float *d_loss_sum, void *stream)
{
    int rc = lk::fx::check_tables(tables, "lk_flexmf_step");
    if (rc != LK_OK) return rc;
    LK_REQUIRE(hyper, "lk_flexmf_step: null hyper-parameters");
    const lk_flexmf_hyper &h = *hyper;
    LK_REQUIRE(h.loss >= LK_FLEXMF_LOGISTIC && h.loss <= LK_FLEXMF_WARP,
               "lk_flexmf_step: unknown loss %d", h.loss);
    LK_REQUIRE(h.optimizer == LK_FLEXMF_ADAMW || h.optimizer == LK_FLEXMF_SPARSE_ADAM,
               "lk_flexmf_step: unknown optimizer %d", h.optimizer);
    LK_REQUIRE(h.n_neg >= 1 && h.n_neg <= 1024, "lk_flexmf_step: n_neg outside 1..1024");
    LK_REQUIRE(h.loss != LK_FLEXMF_WARP || (h.n_neg == 1 && d_weights),
               "lk_flexmf_step: WARP takes one negative and the sample weights");
    LK_REQUIRE(batch >= 1 && batch * (1 + (int64_t)h.n_neg) < ((int64_t)1 << 31),
               "lk_flexmf_step: bad batch size");
    LK_REQUIRE(d_users && d_pos && d_neg && d_ws && d_loss, "lk_flexmf_step: null pointer");
    LK_REQUIRE(h.optimizer != LK_FLEXMF_ADAMW || d_slot, "lk_flexmf_step: AdamW needs d_slot");
    LK_REQUIRE(h.bias_corr1 > 0.0 && h.bias_corr2 > 0.0, "lk_flexmf_step: bad bias correction");
    for (int t = 0; t < 4; ++t)
        LK_REQUIRE(!tables->param[t] || (tables->exp_avg[t] && tables->exp_avg_sq[t]),
                   "lk_flexmf_step: table %d has no optimiser state", t);
    const lk::fx::Scalars H = lk::fx::scalars_of(h);
    const bool aw = h.optimizer == LK_FLEXMF_ADAMW;
    hipStream_t st = lk::as_stream(stream);
    const int kr = (tables->k + 63) / 64;
    if (kr == 1)
        return lk::fx::step_impl<1>(*tables, H, aw, d_users, d_pos, d_neg, d_weights, batch, d_ws,
                                    d_slot, d_loss, d_loss_sum, st);
    if (kr == 2)
        return lk::fx::step_impl<2>(*tables, H, aw, d_users, d_pos, d_neg, d_weights, batch, d_ws,
                                    d_slot, d_loss, d_loss_sum, st);
    return lk::fx::step_impl<4>(*tables, H, aw, d_users, d_pos, d_neg, d_weights, batch, d_ws,
                                d_slot, d_loss, d_loss_sum, st);
}

extern "C" int lk_flexmf_gather_values(const int32_t *d_perm, int64_t n, const float *d_all,
                                       float *d_out, void *stream)
{
    LK_REQUIRE(n >= 0, "lk_flexmf_gather_values: bad length");
    if (n == 0) return LK_OK;
    LK_REQUIRE(d_perm && d_all && d_out, "lk_flexmf_gather_values: null pointer");
    hipLaunchKernelGGL(lk::fx::flexmf_gather_values_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, lk::as_stream(stream), d_perm, n, d_all, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" size_t lk_flexmf_step_explicit_workspace_bytes(int64_t batch, int32_t k)
{
    if (batch < 1 || k < 1 || k > LK_FLEXMF_MAX_K) return 0;
    return lk::fx::layout(nullptr, batch, 0, k, nullptr);
}

extern "C" int lk_flexmf_step_explicit(const lk_flexmf_tables *tables,
                                       const lk_flexmf_hyper *hyper, const int32_t *d_users,
                                       const int32_t *d_items, const float *d_ratings,
                                       int64_t batch, void *d_ws, int32_t *d_slot, float *d_loss,
                                       float *d_loss_sum, void *stream)
{
    int rc = lk::fx::check_tables(tables, "lk_flexmf_step_explicit");
    if (rc != LK_OK) return rc;
    LK_REQUIRE(hyper, "lk_flexmf_step_explicit: null hyper-parameters");
    const lk_flexmf_hyper &h = *hyper;
    LK_REQUIRE(h.loss == LK_FLEXMF_MSE && h.n_neg == 0,
               "lk_flexmf_step_explicit: takes loss LK_FLEXMF_MSE and n_neg 0 (got %d, %d)",
               h.loss, h.n_neg);
    LK_REQUIRE(h.optimizer == LK_FLEXMF_ADAMW || h.optimizer == LK_FLEXMF_SPARSE_ADAM,
               "lk_flexmf_step_explicit: unknown optimizer %d", h.optimizer);
    LK_REQUIRE(batch >= 1 && batch < ((int64_t)1 << 30), "lk_flexmf_step_explicit: bad batch size");
    LK_REQUIRE(d_users && d_items && d_ratings && d_ws && d_loss,
               "lk_flexmf_step_explicit: null pointer");
    LK_REQUIRE(h.optimizer != LK_FLEXMF_ADAMW || d_slot,
               "lk_flexmf_step_explicit: AdamW needs d_slot");
    LK_REQUIRE(h.bias_corr1 > 0.0 && h.bias_corr2 > 0.0,
               "lk_flexmf_step_explicit: bad bias correction");
    for (int t = 0; t < 4; ++t)
        LK_REQUIRE(!tables->param[t] || (tables->exp_avg[t] && tables->exp_avg_sq[t]),
                   "lk_flexmf_step_explicit: table %d has no optimiser state", t);
    const lk::fx::Scalars H = lk::fx::scalars_of(h);
    const bool aw = h.optimizer == LK_FLEXMF_ADAMW;
    hipStream_t st = lk::as_stream(stream);
    const int kr = (tables->k + 63) / 64;
    if (kr == 1)
        return lk::fx::step_mse_impl<1>(*tables, H, aw, d_users, d_items, d_ratings, batch, d_ws,
                                        d_slot, d_loss, d_loss_sum, st);
    if (kr == 2)
        return lk::fx::step_mse_impl<2>(*tables, H, aw, d_users, d_items, d_ratings, batch, d_ws,
                                        d_slot, d_loss, d_loss_sum, st);
    return lk::fx::step_mse_impl<4>(*tables, H, aw, d_users, d_items, d_ratings, batch, d_ws,
                                    d_slot, d_loss, d_loss_sum, st);
}
