// slim.hip -- SLIM / fsSLIM on the device: the coordinate-descent trainer and the batched scorer.
//
// Replaces `lenskit._accel.slim.train_slim` (src/accel/slim/mod.rs:58-301) and the SciPy product
// of `SLIMScorer.__call__` (src/lenskit/knn/slim.py:121-152).
//
// TRAINING.  One elastic-net regression per target item i ("column"), independent of every other
// column; ONE WAVE owns a column from its first user to its last weight, and a persistent grid of
// one-wave workgroups draws columns from a ticket counter.  The contract is the reference's bits,
// so inside a column every step keeps the reference's order:
//   1. active list (`prep_resid_and_active`, mod.rs:196-215): the users of i in stored order, each
//      user's items in stored order, 64 items to the instruction.  The items of one user are
//      distinct, so the lanes of a chunk never meet on a counter: the co-rating count is a plain
//      read-modify-write, and an item joins the list where a ballot of "count was 0" puts it --
//      first-encounter order without a sort.
//   2. fsSLIM cut (mod.rs:217-231): key = -(count_j) / (sqrt(n_i) * sqrt(n_j)) in float64 -- the
//      square roots come from a host table, the multiply and the divide are IEEE here --, turned
//      into an order-preserving 64-bit integer and sorted by a wave-local LSD radix sort, eight
//      bits a pass.  Every pass is stable (a key's rank inside its 64-key chunk from a match mask
//      of eight ballots, chunks in order), so equal keys keep first-encounter order like Rust's
//      `sort_by_key`.  A pass whose digit is the same for the whole list is skipped.
//   3. coordinate descent (`cd_single`, mod.rs:267-290): per coordinate j the gather of resid[u],
//      the inner `+ w_j` and the `resid -= diff` scatter are lane-parallel (the users of one item
//      are distinct); the running float32 sum is the one sequential chain -- v_readlane + v_add
//      per entry, all lanes carrying the same value.  The (item, offset, length, weight) of 64
//      coordinates are loaded lane-parallel and handed out by readlane; the first users of the
//      next coordinate are fetched while the current chain runs.  A coordinate whose weight did
//      not move (diff == 0: x - 0 is x) skips the scatter.
//   4. output (mod.rs:162-172): the kept weights go back to their items' cells, one ascending scan
//      over the items compacts those >= 1e-12 into the column's staging row.
// The residual vector lives in LDS up to SLIM_LDS_USERS users and in the wave's slot of the
// workspace beyond (ML-25M: 162 541 users); it is cleared by a plain fill after each column.
//
// SCORING.  A workgroup per query adds the history items' weight rows to the query's row of a
// dense panel, one history item after the other (SciPy's order for `x @ weights`); the targets
// inside one weight row are distinct.
#include "common.h"

namespace lk {

constexpr int SLIM_LDS_USERS = 4096;  // residuals in LDS up to here (16 KiB a wave)
constexpr float SLIM_EPSILON = 1.0e-12f;       // mod.rs:27
constexpr float SLIM_OPT_TOLERANCE = 1e-3f;    // mod.rs:28

__device__ __forceinline__ int rl_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float rl_f(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ int64_t rl_p(int64_t v, int lane)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((uint64_t)v >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t rl_p(int32_t v, int lane) { return rl_i(v, lane); }

// layout of one wave's slot in the workspace (elements padded to a multiple of four)
struct SlimSlot {
    int64_t ni4, nu4;
    size_t bytes;
    __host__ __device__ SlimSlot(int64_t n_users, int64_t n_items, bool resid_in_lds)
    {
        ni4 = (n_items + 3) / 4 * 4;
        nu4 = resid_in_lds ? 0 : (n_users + 3) / 4 * 4;
        bytes = ((size_t)ni4 * 24 + (size_t)nu4 * 4 + 255) / 256 * 256;
    }
};

struct SlimHeader {  // first 256 bytes of the workspace
    int ticket;
    int pad;
    unsigned long long rounds, coords, entries;
};

template <bool IS64, bool RLDS, bool CTL>
__global__ __launch_bounds__(64) void slim_train_kernel(
    const typename IndPtr<IS64>::type *__restrict__ ui_ptr, const int32_t *__restrict__ ui_idx,
    const typename IndPtr<IS64>::type *__restrict__ iu_ptr, const int32_t *__restrict__ iu_idx,
    const double *__restrict__ item_sqrt, int32_t n_users, int32_t n_items,
    const int32_t *__restrict__ columns, int32_t n_cols, float l1, float l2, int32_t max_iters,
    int32_t max_nbrs, char *slots, SlimHeader *hdr, int32_t cap, int32_t *st_idx, float *st_val,
    int32_t *counts, TaskCtlDev ctl)
{
    using IT = typename IndPtr<IS64>::type;
    extern __shared__ __attribute__((aligned(16))) float lds_resid[];
    __shared__ unsigned hist[256];
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const SlimSlot lay(n_users, n_items, RLDS);
    char *slot = slots + (size_t)blockIdx.x * lay.bytes;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(slot);
    int32_t *cnt = reinterpret_cast<int32_t *>(key + lay.ni4);
    int32_t *act0 = cnt + lay.ni4;
    int32_t *act1 = act0 + lay.ni4;
    float *wact = reinterpret_cast<float *>(act1 + lay.ni4);
    float *resid = RLDS ? lds_resid : wact + lay.ni4;

    for (int j = lane; j < n_items; j += 64) cnt[j] = 0;
    for (int u = lane; u < n_users; u += 64) resid[u] = 0.f;
    wave_lds_sync();

    unsigned long long s_rounds = 0ull, s_coords = 0ull, s_entries = 0ull;
    for (;;) {
        int ci = 0;
        if (lane == 0) ci = atomicAdd(&hdr->ticket, 1);
        ci = __builtin_amdgcn_readfirstlane(ci);
        if (ci >= n_cols) break;
        if (CTL) {  // AccelTask.cancel: columns not started keep their zero count
            int c = 0;
            if (lane == 0) c = ctl_cancelled(ctl, (ci & 63) == 0) ? 1 : 0;
            if (__builtin_amdgcn_readfirstlane(c)) break;
        }
        const int i = columns ? columns[ci] : ci;
        const IT ib = iu_ptr[i], ie = iu_ptr[i + 1];

        // ---- 1. residuals + active list in first-encounter order, co-rating counts ----------
        int L = 0;
        for (IT p0 = ib; p0 < ie; p0 += 64) {
            const bool okp = p0 + lane < ie;
            const int u_l = okp ? iu_idx[p0 + lane] : 0;
            const IT ub_l = ui_ptr[u_l];
            const int un_l = (int)(ui_ptr[u_l + 1] - ub_l);
            if (okp) resid[u_l] = 1.0f;
            const int m = (int)((ie - p0) < 64 ? (ie - p0) : 64);
            for (int t = 0; t < m; ++t) {
                const int64_t ub = rl_p(ub_l, t);
                const int un = rl_i(un_l, t);
                for (int q = 0; q < un; q += 64) {
                    const bool ok = q + lane < un;
                    const int j = ok ? ui_idx[ub + q + lane] : i;
                    const bool live = j != i;
                    const int c = live ? cnt[j] : 1;
                    const bool first = c == 0;
                    const unsigned long long mk = __builtin_amdgcn_ballot_w64(first);
                    if (first) act0[L + __popcll(mk & lt)] = j;
                    if (live) cnt[j] = c + 1;
                    L += __popcll(mk);
                    wave_lds_sync();  // the next chunk (another user) reads these counters
                }
            }
        }

        // ---- 2. fsSLIM: stable sort by cosine key, keep the first max_nbrs ------------------
        int32_t *act = act0;
        int K = L;
        if (max_nbrs > 0 && max_nbrs < L) {
            const double inorm = item_sqrt[i];
            for (int pos = lane; pos < L; pos += 64) {
                const int j = act0[pos];
                const double k = -(double)cnt[j] / (inorm * item_sqrt[j]);
                // every key is negative: ascending value = descending magnitude = ascending ~bits
                key[j] = ~__builtin_bit_cast(unsigned long long, k);
            }
            wave_lds_sync();
            int32_t *src = act0, *dst = act1;
            for (int shift = 0; shift < 64; shift += 8) {
                for (int d = lane; d < 256; d += 64) hist[d] = 0u;
                wave_lds_sync();
                for (int pos = lane; pos < L; pos += 64)
                    atomicAdd(&hist[(unsigned)(key[src[pos]] >> shift) & 255u], 1u);
                wave_lds_sync();
                // exclusive scan of the 256 counts, four per lane
                unsigned a[4], s = 0u;
                bool whole = false;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    a[b] = hist[lane * 4 + b];
                    whole |= a[b] == (unsigned)L;
                    s += a[b];
                }
                if (__builtin_amdgcn_ballot_w64(whole) != 0ull) continue;  // one digit: no move
                unsigned incl = s;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                unsigned run = incl - s;
                wave_lds_sync();
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    hist[lane * 4 + b] = run;
                    run += a[b];
                }
                wave_lds_sync();
                for (int p0 = 0; p0 < L; p0 += 64) {
                    const bool ok = p0 + lane < L;
                    const int j = ok ? src[p0 + lane] : 0;
                    const unsigned d = ok ? ((unsigned)(key[j] >> shift) & 255u) : 0u;
                    unsigned long long peers = __builtin_amdgcn_ballot_w64(ok);
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const bool bit = (d >> b) & 1u;
                        const unsigned long long mk = __builtin_amdgcn_ballot_w64(bit);
                        peers &= bit ? mk : ~mk;
                    }
                    const unsigned base = ok ? hist[d] : 0u;
                    if (ok) dst[base + __popcll(peers & lt)] = j;
                    wave_lds_sync();
                    if (ok && (peers & lt) == 0ull) hist[d] = base + (unsigned)__popcll(peers);
                    wave_lds_sync();
                }
                int32_t *tmp = src;
                src = dst;
                dst = tmp;
            }
            act = src;
            K = max_nbrs;
        }

        // ---- 3. coordinate descent ----------------------------------------------------------
        for (int pos = lane; pos < K; pos += 64) wact[pos] = 0.f;
        wave_lds_sync();
        unsigned long long col_entries = 0ull;
        int rounds = 0;
        for (int it = 0; it < max_iters; ++it) {
            float dmax = 0.f;
            unsigned long long ent = 0ull;
            for (int p0 = 0; p0 < K; p0 += 64) {
                const bool okp = p0 + lane < K;
                const int j_l = okp ? act[p0 + lane] : 0;
                const IT b_l = iu_ptr[j_l];
                const int n_l = okp ? (int)(iu_ptr[j_l + 1] - b_l) : 0;
                float w_l = okp ? wact[p0 + lane] : 0.f;
                const int m = (K - p0) < 64 ? (K - p0) : 64;
                // the first users of coordinate 0; inside the loop always one coordinate ahead
                int u_pre = 0;
                {
                    const int64_t b = rl_p(b_l, 0);
                    if (lane < rl_i(n_l, 0)) u_pre = iu_idx[b + lane];
                }
                for (int t = 0; t < m; ++t) {
                    const int64_t b = rl_p(b_l, t);
                    const int n = rl_i(n_l, t);
                    const float w = rl_f(w_l, t);
                    const int u0 = u_pre;
                    if (t + 1 < m) {
                        const int64_t b2 = rl_p(b_l, t + 1);
                        u_pre = (lane < rl_i(n_l, t + 1)) ? iu_idx[b2 + lane] : 0;
                    }
                    float upd = 0.f;
                    for (int c0 = 0; c0 < n; c0 += 64) {
                        const bool ok = c0 + lane < n;
                        const int u = c0 == 0 ? u0 : (ok ? iu_idx[b + c0 + lane] : 0);
                        const float r = ok ? resid[u] + w : 0.f;
                        const int mm = (n - c0) < 64 ? (n - c0) : 64;
                        if (mm == 64) {
#pragma unroll
                            for (int s = 0; s < 64; ++s) upd += rl_f(r, s);
                        } else {
                            for (int s = 0; s < mm; ++s) upd += rl_f(r, s);
                        }
                    }
                    float nw = 0.f;
                    if (upd >= l1) nw = (upd - l1) / ((float)n + l2);  // soft_thresh, mod.rs:292
                    const float diff = nw - w;
                    if (diff != 0.f) {
                        for (int c0 = 0; c0 < n; c0 += 64) {
                            const bool ok = c0 + lane < n;
                            const int u = c0 == 0 ? u0 : (ok ? iu_idx[b + c0 + lane] : 0);
                            if (ok) resid[u] -= diff;
                        }
                        wave_lds_sync();  // the next coordinate's users may be these
                    }
                    if (lane == t) w_l = nw;
                    const float ad = fabsf(diff);
                    if (ad > dmax) dmax = ad;
                    ent += (unsigned)n;
                }
                if (okp) wact[p0 + lane] = w_l;
            }
            wave_lds_sync();
            ++rounds;
            col_entries += ent;
            if (dmax <= SLIM_OPT_TOLERANCE) break;
        }
        s_rounds += (unsigned)rounds;
        s_coords += (unsigned long long)rounds * (unsigned)K;
        s_entries += col_entries;

        // ---- 4. the column's row: weights >= EPSILON by ascending item ----------------------
        for (int pos = lane; pos < L; pos += 64)
            cnt[act[pos]] = pos < K ? __builtin_bit_cast(int, wact[pos]) : 0;
        wave_lds_sync();
        int32_t *oi = st_idx + (size_t)ci * cap;
        float *ov = st_val + (size_t)ci * cap;
        int out = 0;
        if (L > 0) {
            for (int j0 = 0; j0 < n_items; j0 += 64) {
                const int j = j0 + lane;
                const float v = j < n_items ? __builtin_bit_cast(float, cnt[j]) : 0.f;
                const bool keep = v >= SLIM_EPSILON;
                const unsigned long long mk = __builtin_amdgcn_ballot_w64(keep);
                if (keep) {
                    const int o = out + __popcll(mk & lt);
                    oi[o] = j;
                    ov[o] = v;
                }
                out += __popcll(mk);
            }
        }
        if (lane == 0) counts[ci] = out;
        // leave the slot as it was found
        for (int pos = lane; pos < L; pos += 64) cnt[act[pos]] = 0;
        if (ie > ib)
            for (int u = lane; u < n_users; u += 64) resid[u] = 0.f;
        wave_lds_sync();
        if (CTL && lane == 0) ctl_advance(ctl, 1);
    }
    if (lane == 0) {
        atomicAdd(&hdr->rounds, s_rounds);
        atomicAdd(&hdr->coords, s_coords);
        atomicAdd(&hdr->entries, s_entries);
    }
}

// out_indptr = exclusive scan of the per-column counts (one workgroup; n_cols <= 2^31)
__global__ __launch_bounds__(256) void slim_scan_kernel(const int32_t *__restrict__ counts,
                                                        int64_t n, int64_t *__restrict__ out)
{
    __shared__ long long part[256];
    const int t = threadIdx.x;
    const int64_t seg = (n + 255) / 256;
    const int64_t b = t * seg < n ? t * seg : n, e = b + seg < n ? b + seg : n;
    long long s = 0;
    for (int64_t i = b; i < e; ++i) s += counts[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < 256; ++k) {
            const long long v = part[k];
            part[k] = run;
            run += v;
        }
        out[n] = run;
    }
    __syncthreads();
    long long run = part[t];
    for (int64_t i = b; i < e; ++i) {
        out[i] = run;
        run += counts[i];
    }
}

__global__ __launch_bounds__(256) void slim_unstage_kernel(
    const int32_t *__restrict__ counts, const int64_t *__restrict__ out_ptr, int64_t cap,
    const int32_t *__restrict__ st_idx, const float *__restrict__ st_val,
    int32_t *__restrict__ out_idx, float *__restrict__ out_val)
{
    const int64_t c = blockIdx.x;
    const int n = counts[c];
    const int64_t o = out_ptr[c];
    for (int k = threadIdx.x; k < n; k += 256) {
        out_idx[o + k] = st_idx[c * cap + k];
        out_val[o + k] = st_val[c * cap + k];
    }
}

// ---- scoring ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slim_score_kernel(
    const int64_t *__restrict__ hist_ptr, const int32_t *__restrict__ hist_items,
    const int64_t *__restrict__ w_ptr, const int32_t *__restrict__ w_idx,
    const float *__restrict__ w_val, int64_t n_items, float *out, int64_t ld_out, int mark)
{
    const int64_t q = blockIdx.x;
    float *row = out + q * ld_out;
    const int64_t hb = hist_ptr[q], he = hist_ptr[q + 1];
    const float nan = __builtin_nanf("");
    const float fill = ((mark & 2) && hb == he) ? nan : 0.f;  // no history: nothing to list
    for (int64_t c = threadIdx.x; c < n_items; c += 256) row[c] = fill;
    __syncthreads();
    for (int64_t h = hb; h < he; ++h) {
        const int32_t it = hist_items[h];
        if (it < 0 || it >= n_items) continue;  // unknown item: dropped (slim.py:133-134)
        const int64_t b = w_ptr[it], e = w_ptr[it + 1];
        for (int64_t k = b + threadIdx.x; k < e; k += 256) row[w_idx[k]] += w_val[k];
        __syncthreads();  // the next history item's row may name the same targets
    }
    if (mark & 1) {  // the query's own items are no candidates
        for (int64_t h = hb + threadIdx.x; h < he; h += 256) {
            const int32_t it = hist_items[h];
            if (it >= 0 && it < n_items) row[it] = nan;
        }
    }
}

__global__ void take_scores_kernel(const float *__restrict__ scores, int64_t n_rows,
                                   int64_t row_len, const int32_t *__restrict__ idx, int64_t n,
                                   float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows * n) return;
    const int32_t c = idx[e];
    out[e] = (c >= 0 && c < row_len) ? scores[(e / n) * row_len + c] : __builtin_nanf("");
}

static int slim_cus()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n <= 0)
            n = 256;
        cus = n;
    }
    return cus;
}

// resident one-wave workgroups of the trainer: LDS residuals bound them per CU
static int64_t slim_slots(int64_t n_users, int64_t n_cols)
{
    const bool rlds = n_users <= SLIM_LDS_USERS;
    int64_t per_cu = 8;
    if (rlds) {
        per_cu = (int64_t)(160 * 1024) / (n_users * 4 + 2048);
        per_cu = per_cu > 16 ? 16 : (per_cu < 1 ? 1 : per_cu);
    }
    const int64_t s = per_cu * slim_cus();
    return n_cols < s ? (n_cols > 0 ? n_cols : 1) : s;
}

struct SlimWs {
    size_t off_counts, off_idx, off_val, off_slots, total;
    int64_t cap, slots;
    SlimWs(int64_t n_users, int64_t n_items, int64_t n_cols, int64_t max_nbrs)
    {
        cap = (max_nbrs > 0 && max_nbrs < n_items) ? max_nbrs : n_items;
        if (cap < 1) cap = 1;
        slots = slim_slots(n_users, n_cols);
        const SlimSlot lay(n_users, n_items, n_users <= SLIM_LDS_USERS);
        size_t o = 256;
        off_counts = o;
        o += align_up((size_t)(n_cols > 0 ? n_cols : 1) * 4, 256);
        off_idx = o;
        o += align_up((size_t)n_cols * (size_t)cap * 4, 256);
        off_val = o;
        o += align_up((size_t)n_cols * (size_t)cap * 4, 256);
        off_slots = o;
        o += (size_t)slots * lay.bytes;
        total = o;
    }
};

}  // namespace lk

extern "C" size_t lk_slim_train_workspace_bytes(int64_t n_users, int64_t n_items, int64_t n_cols,
                                                int64_t max_nbrs)
{
    if (n_users < 0 || n_items < 0 || n_cols < 0) return 0;
    return lk::SlimWs(n_users, n_items, n_cols, max_nbrs).total;
}

extern "C" int lk_slim_train_count(const void *d_ui_indptr, const int32_t *d_ui_indices,
                                   const void *d_iu_indptr, const int32_t *d_iu_indices,
                                   int indptr_is_64, int64_t n_users, int64_t n_items,
                                   const double *d_item_sqrt, float l1_reg, float l2_reg,
                                   int32_t max_iters, int64_t max_nbrs, const int32_t *d_columns,
                                   int64_t n_cols, lk_task_ctl *ctl, void *d_ws,
                                   int64_t *d_out_indptr, int64_t *h_total_nnz, int64_t *h_stats,
                                   void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_cols >= 0 && n_users < ((int64_t)1 << 31) - 64 &&
                   n_items < ((int64_t)1 << 31) - 64 && n_cols < ((int64_t)1 << 31) - 64,
               "lk_slim_train_count: bad shape");
    LK_REQUIRE(max_iters >= 1, "lk_slim_train_count: max_iters must be positive");
    LK_REQUIRE(d_columns || n_cols == n_items,
               "lk_slim_train_count: without a column list n_cols must be n_items");
    LK_REQUIRE(d_out_indptr && h_total_nnz, "lk_slim_train_count: null output");
    hipStream_t st = as_stream(stream);
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = 0;
    if (n_cols == 0) {
        LK_HIP_CHECK(hipMemsetAsync(d_out_indptr, 0, sizeof(int64_t), st));
        LK_HIP_CHECK(hipStreamSynchronize(st));
        *h_total_nnz = 0;
        return LK_OK;
    }
    LK_REQUIRE(d_ui_indptr && d_iu_indptr && d_item_sqrt && d_ws,
               "lk_slim_train_count: null pointer");
    const SlimWs w(n_users, n_items, n_cols, max_nbrs);
    char *ws = static_cast<char *>(d_ws);
    SlimHeader *hdr = reinterpret_cast<SlimHeader *>(ws);
    int32_t *counts = reinterpret_cast<int32_t *>(ws + w.off_counts);
    LK_HIP_CHECK(hipMemsetAsync(ws, 0, w.off_idx, st));  // header + counts
    if (ctl) {
        int rc = ctl_begin(ctl, n_cols, n_cols, st);
        if (rc != LK_OK) return rc;
    }
    const bool rlds = n_users <= SLIM_LDS_USERS;
    const size_t lds = rlds ? align_up((size_t)(n_users > 0 ? n_users : 1) * 4, 16) : 0;
    const int32_t mn = (max_nbrs > 0 && max_nbrs < n_items) ? (int32_t)max_nbrs : 0;
#define LK_SLIM_LAUNCH(IS64, RLDS, CTL)                                                          \
    hipLaunchKernelGGL((slim_train_kernel<IS64, RLDS, CTL>), dim3((unsigned)w.slots), dim3(64),  \
                       lds, st, static_cast<const IndPtr<IS64>::type *>(d_ui_indptr),            \
                       d_ui_indices, static_cast<const IndPtr<IS64>::type *>(d_iu_indptr),       \
                       d_iu_indices, d_item_sqrt, (int32_t)n_users, (int32_t)n_items, d_columns, \
                       (int32_t)n_cols, l1_reg, l2_reg, max_iters, mn, ws + w.off_slots, hdr,    \
                       (int32_t)w.cap, reinterpret_cast<int32_t *>(ws + w.off_idx),              \
                       reinterpret_cast<float *>(ws + w.off_val), counts,                        \
                       ctl ? ctl->dev() : TaskCtlDev{})
#define LK_SLIM_LAUNCH2(IS64, RLDS)                  \
    do {                                             \
        if (ctl)                                     \
            LK_SLIM_LAUNCH(IS64, RLDS, true);        \
        else                                         \
            LK_SLIM_LAUNCH(IS64, RLDS, false);       \
    } while (0)
    if (indptr_is_64) {
        if (rlds)
            LK_SLIM_LAUNCH2(true, true);
        else
            LK_SLIM_LAUNCH2(true, false);
    } else {
        if (rlds)
            LK_SLIM_LAUNCH2(false, true);
        else
            LK_SLIM_LAUNCH2(false, false);
    }
#undef LK_SLIM_LAUNCH2
#undef LK_SLIM_LAUNCH
    hipLaunchKernelGGL(slim_scan_kernel, dim3(1), dim3(256), 0, st, counts, n_cols, d_out_indptr);
    LK_HIP_CHECK(hipGetLastError());
    LK_HIP_CHECK(hipMemcpyAsync(h_total_nnz, d_out_indptr + n_cols, sizeof(int64_t),
                                hipMemcpyDeviceToHost, st));
    SlimHeader h;
    LK_HIP_CHECK(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = (int64_t)h.rounds;
        h_stats[1] = (int64_t)h.coords;
        h_stats[2] = (int64_t)h.entries;
    }
    if (ctl) return ctl_finish(ctl, st);  // LK_E_CANCELLED if interrupted
    return LK_OK;
}

extern "C" int lk_slim_train_fill(int64_t n_users, int64_t n_items, int64_t n_cols,
                                  int64_t max_nbrs, const void *d_ws, const int64_t *d_out_indptr,
                                  int32_t *d_out_indices, float *d_out_values, void *stream)
{
    using namespace lk;
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_cols >= 0, "lk_slim_train_fill: bad shape");
    if (n_cols == 0 || !d_out_indices || !d_out_values) return LK_OK;  // nothing survived
    LK_REQUIRE(d_ws && d_out_indptr, "lk_slim_train_fill: null pointer");
    const SlimWs w(n_users, n_items, n_cols, max_nbrs);
    const char *ws = static_cast<const char *>(d_ws);
    hipLaunchKernelGGL(slim_unstage_kernel, dim3((unsigned)n_cols), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const int32_t *>(ws + w.off_counts), d_out_indptr, w.cap,
                       reinterpret_cast<const int32_t *>(ws + w.off_idx),
                       reinterpret_cast<const float *>(ws + w.off_val), d_out_indices,
                       d_out_values);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_slim_score_batch(const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                                   int64_t n_queries, const int64_t *d_w_indptr,
                                   const int32_t *d_w_indices, const float *d_w_values,
                                   int64_t n_items, float *d_out, int64_t ld_out,
                                   int mark_history, void *stream)
{
    LK_REQUIRE(n_queries >= 0 && n_items >= 0 && ld_out >= n_items &&
                   n_queries < ((int64_t)1 << 31),
               "lk_slim_score_batch: bad shape");
    if (n_queries == 0 || n_items == 0) return LK_OK;
    LK_REQUIRE(d_hist_ptr && d_w_indptr && d_out, "lk_slim_score_batch: null pointer");
    hipLaunchKernelGGL(lk::slim_score_kernel, dim3((unsigned)n_queries), dim3(256), 0,
                       lk::as_stream(stream), d_hist_ptr, d_hist_items, d_w_indptr, d_w_indices,
                       d_w_values, n_items, d_out, ld_out, mark_history);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

extern "C" int lk_take_scores(const float *d_scores, int64_t n_rows, int64_t row_len,
                              const int32_t *d_idx, int64_t n, float *d_out, void *stream)
{
    LK_REQUIRE(n_rows >= 0 && row_len >= 0 && n >= 0, "lk_take_scores: bad shape");
    if (n_rows == 0 || n == 0) return LK_OK;
    LK_REQUIRE(d_scores && d_idx && d_out, "lk_take_scores: null pointer");
    const int64_t total = n_rows * n;
    hipLaunchKernelGGL(lk::take_scores_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       lk::as_stream(stream), d_scores, n_rows, row_len, d_idx, n, d_out);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}
