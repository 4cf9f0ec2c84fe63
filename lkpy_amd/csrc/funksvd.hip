// funksvd.hip -- the FunkSVD trainer on gfx950 (`FunkSVDScorer.train`, src/lenskit/funksvd.py:111-197,
// whose epoch is `FunkSVDTrainer::feature_epoch`, src/accel/funksvd.rs:67-128).
//
// The reference walks the shuffled samples one after the other.  A sample (u, i, r) reads and writes
// only column entry u of the user factors and entry i of the item factors, so two samples that
// share neither commute exactly, and the walk is a DAG:
//     level(s) = 1 + max(level of the previous sample of u, level of the previous sample of i).
// All samples of a level may run at once, and every float32 the reference stores is reproduced.
//
// lk_funksvd_plan_levels / lk_funksvd_plan_order (host): the levels in one sequential pass, then a
//   stable counting sort by level and the marks of the NARROW RUNS -- runs of consecutive levels
//   of at most 64 samples each, as long as they can be with at most STAGE samples in a run.
//
// lk_funksvd_train_feature: ONE workgroup of 1024 threads runs `epochs` epochs of one feature over
//   the level-ordered samples.  Lane t takes the samples t, t + 1024, ... of a level and a block
//   barrier separates two levels; the first entries of the next level are fetched before the
//   barrier.  The feature's two columns sit in LDS where they fit LDS_COLUMN_BYTES and in global
//   memory otherwise (one barrier a level there).  With the columns in LDS, a narrow run's
//   samples are first copied into LDS by all waves; then wave 0 walks the run alone, one sample
//   per lane, with a workgroup-scope fence between two levels and no barrier -- nothing but LDS
//   is read between two fences, the next level's samples before the fence -- while the other
//   waves wait once, at the end of the run.  The arithmetic of a sample is the reference's, one
//   IEEE double operation per operation, nothing contracted.
#include <vector>

#include "common.h"

namespace lk {
namespace funksvd {

constexpr int THREADS = 1024;
constexpr int NARROW = 64;  // a level this wide or narrower fits one wave
// -DLK_FUNKSVD_NARROW_RUNS=0 builds the kernel without the narrow-run walk (every level ends in a
// block barrier): the yardstick tools/funksvd_time.py times the walk against.
#ifndef LK_FUNKSVD_NARROW_RUNS
#define LK_FUNKSVD_NARROW_RUNS 1
#endif
constexpr bool NARROW_RUNS = LK_FUNKSVD_NARROW_RUNS != 0;
constexpr int STAGE = 2048;  // samples of a narrow run staged in LDS (32 KiB)
// The columns' LDS budget: 112 KiB of the 160 KiB a workgroup may declare; the stage and the
// reduction scratch (32 + 8 KiB, static) sit beside it.
constexpr size_t LDS_COLUMN_BYTES = 112 * 1024;

struct __attribute__((aligned(16))) Sample {
    int32_t u, i;
    float r, est;
};

__device__ __forceinline__ Sample fetch(const int32_t *users, const int32_t *items,
                                        const float *ratings, const float *est, int64_t p,
                                        int64_t hi)
{
    Sample s = {0, 0, 0.0f, 0.0f};
    if (p < hi) {
        s.u = users[p];
        s.i = items[p];
        s.r = ratings[p];
        s.est = est[p];
    }
    return s;
}

// funksvd.rs:98-124 for one sample; returns the squared error
__device__ __forceinline__ double update(float *ucol, float *icol, const Sample &s, int32_t n_users,
                                         int32_t n_items, double lr, double reg, double trail,
                                         double rmin, double rmax)
{
#pragma clang fp contract(off)
    if ((uint32_t)s.u >= (uint32_t)n_users || (uint32_t)s.i >= (uint32_t)n_items) return 0.0;
    const double ufv = (double)ucol[s.u];
    const double ifv = (double)icol[s.i];
    const double prod = ufv * ifv;
    double pred = (double)s.est + prod;
    pred = pred + trail;
    if (pred < rmin) pred = rmin;  // f64::clamp: a NaN passes through
    if (pred > rmax) pred = rmax;
    const double err = (double)s.r - pred;
    const double ea = err * ifv, ra = reg * ufv;
    const double ufd = (ea - ra) * lr;
    const double eb = err * ufv, rb = reg * ifv;
    const double ifd = (eb - rb) * lr;
    ucol[s.u] = (float)(ufv + ufd);
    icol[s.i] = (float)(ifv + ifd);
    return err * err;
}

__device__ __forceinline__ void level_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void train_feature_kernel(
    const int32_t *__restrict__ users, const int32_t *__restrict__ items,
    const float *__restrict__ ratings, float *est, const int64_t *__restrict__ level_ptr,
    const int32_t *__restrict__ run_end, int32_t depth, float *g_ucol, float *g_icol,
    int32_t n_users, int32_t n_items, int32_t epochs, int32_t finish, double lr, double reg,
    double trail, double rmin, double rmax, double *__restrict__ sse)
{
#pragma clang fp contract(off)
    // Narrow runs are walked where the columns sit in LDS.  With the columns in global memory
    // the walk measured slower than a barrier a level at the ML-25M shape, so that
    // regime has none.
    constexpr bool RUNS = NARROW_RUNS && LDS;
    extern __shared__ float lds_cols[];
    __shared__ double red[THREADS];
    __shared__ Sample stage[RUNS ? STAGE : 1];
    const int tid = threadIdx.x;
    float *ucol, *icol;
    if constexpr (LDS) {
        ucol = lds_cols;
        icol = lds_cols + n_users;
        for (int p = tid; p < n_users; p += THREADS) ucol[p] = g_ucol[p];
        for (int p = tid; p < n_items; p += THREADS) icol[p] = g_icol[p];
    } else {
        ucol = g_ucol;
        icol = g_icol;
    }
    __syncthreads();
    const int64_t n = level_ptr[depth];

    for (int e = 0; e < epochs; ++e) {
        double part = 0.0;
        // level L is [lo, hi), level L + 1 is [hi, nhi); re and nre are their run marks.  The
        // offsets and marks are held two levels ahead, so that a level never begins by waiting
        // for a scalar load.
        int64_t lo = 0;
        int64_t hi = depth > 0 ? level_ptr[1] : 0;
        int64_t nhi = depth > 1 ? level_ptr[2] : hi;
        Sample s = fetch(users, items, ratings, est, lo + tid, hi);
        int L = 0;
        int re = RUNS && depth > 0 ? run_end[0] : 0;
        int nre = RUNS && depth > 1 ? run_end[1] : 1;
        while (L < depth) {
            if (RUNS && re > L) {
                // a narrow run [L, re), at most STAGE samples: all waves copy them into LDS, then
                // wave 0 walks alone, one sample per lane, fences between levels
                const int64_t end = level_ptr[re];
                for (int64_t p = lo + tid; p < end && p - lo < STAGE; p += THREADS)
                    stage[p - lo] = fetch(users, items, ratings, est, p, end);
                __syncthreads();
                if (tid < WAVE) {
                    for (int l0 = L; l0 < re; l0 += WAVE - 1) {
                        // lane j holds where level l0 + j starts in the stage
                        const int lj = l0 + tid < re ? l0 + tid : re;
                        const int off = (int)(level_ptr[lj] - lo);
                        const int cnt = re - l0 < WAVE - 1 ? re - l0 : WAVE - 1;
                        int a = __builtin_amdgcn_readlane(off, 0);
                        Sample nxt = stage[a + tid < STAGE ? a + tid : STAGE - 1];
                        for (int j = 0; j < cnt; ++j) {
                            const int b = __builtin_amdgcn_readlane(off, j + 1);
                            const bool mine = a + tid < b;
                            const Sample cur = nxt;
                            nxt = stage[b + tid < STAGE ? b + tid : STAGE - 1];
                            if (mine)
                                part += update(ucol, icol, cur, n_users, n_items, lr, reg, trail,
                                               rmin, rmax);
                            level_fence();
                            a = b;
                        }
                    }
                }
                __syncthreads();
                L = re;  // everybody picks the walk up behind the run
                lo = end;
                hi = L < depth ? level_ptr[L + 1] : lo;
                nhi = L + 1 < depth ? level_ptr[L + 2] : hi;
                re = L < depth ? run_end[L] : L;
                nre = L + 1 < depth ? run_end[L + 1] : L + 1;
                s = fetch(users, items, ratings, est, lo + tid, hi);
            } else {
                // asked for before the barrier: the offset and mark two levels on, and the first
                // entries of the next level
                const int64_t nnhi = L + 2 < depth ? level_ptr[L + 3] : nhi;
                const int nnre = RUNS && L + 2 < depth ? run_end[L + 2] : L + 2;
                const bool mine = lo + tid < hi;
                const Sample cur = s;
                s = fetch(users, items, ratings, est, hi + tid, nhi);
                if (mine)
                    part += update(ucol, icol, cur, n_users, n_items, lr, reg, trail, rmin, rmax);
                for (int64_t p = lo + tid + THREADS; p < hi; p += THREADS)
                    part += update(ucol, icol, fetch(users, items, ratings, est, p, hi), n_users,
                                   n_items, lr, reg, trail, rmin, rmax);
                __syncthreads();
                lo = hi;
                hi = nhi;
                nhi = nnhi;
                re = nre;
                nre = nnre;
                ++L;
            }
        }
        // the epoch's squared error: the lanes' partial sums through a fixed tree
        red[tid] = part;
        __syncthreads();
        for (int o = THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) sse[e] = red[0];
        __syncthreads();
    }

    if (finish) {
        // funksvd.py:188-190: est = clip(est + uemb[users, f] * iemb[items, f], rmin, rmax) in
        // float32, the product and the sum rounded separately
        const float fmin = (float)rmin, fmax = (float)rmax;
        for (int64_t p = tid; p < n; p += THREADS) {
            const int32_t u = users[p], i = items[p];
            if ((uint32_t)u >= (uint32_t)n_users || (uint32_t)i >= (uint32_t)n_items) continue;
            const float prod = ucol[u] * icol[i];
            float v = est[p] + prod;
            if (v < fmin) v = fmin;
            if (v > fmax) v = fmax;
            est[p] = v;
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int p = tid; p < n_users; p += THREADS) g_ucol[p] = ucol[p];
        for (int p = tid; p < n_items; p += THREADS) g_icol[p] = icol[p];
    }
}

template <bool LDS>
static int launch(const int32_t *users, const int32_t *items, const float *ratings, float *est,
                  const int64_t *level_ptr, const int32_t *run_end, int32_t depth, float *ucol,
                  float *icol, int32_t n_users, int32_t n_items, int32_t epochs, int32_t finish,
                  double lr, double reg, double trail, double rmin, double rmax, double *sse,
                  hipStream_t st)
{
    size_t lds = 0;
    if (LDS) {
        lds = ((size_t)n_users + (size_t)n_items) * sizeof(float);
        static lk::PerDeviceOnce attr_once;
        bool &attr_set = attr_once.flag();
        if (!attr_set) {
            LK_HIP_CHECK(hipFuncSetAttribute(
                reinterpret_cast<const void *>(&train_feature_kernel<LDS>),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_COLUMN_BYTES));
            attr_set = true;
        }
    }
    hipLaunchKernelGGL((train_feature_kernel<LDS>), dim3(1), dim3(THREADS), lds, st,
                       users, items, ratings, est, level_ptr, run_end, depth, ucol, icol, n_users,
                       n_items, epochs, finish, lr, reg, trail, rmin, rmax, sse);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

}  // namespace funksvd
}  // namespace lk

extern "C" int32_t lk_funksvd_narrow_width(void) { return lk::funksvd::NARROW; }

extern "C" int32_t lk_funksvd_stage_samples(void) { return lk::funksvd::STAGE; }

extern "C" size_t lk_funksvd_lds_column_bytes(void) { return lk::funksvd::LDS_COLUMN_BYTES; }

extern "C" int lk_funksvd_plan_levels(const int32_t *users, const int32_t *items, int64_t n,
                                      int64_t n_users, int64_t n_items, int32_t *level,
                                      int32_t *depth)
{
    LK_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "lk_funksvd_plan_levels: n = %lld outside 0..2^31",
               (long long)n);
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_users < ((int64_t)1 << 31) &&
                   n_items < ((int64_t)1 << 31),
               "lk_funksvd_plan_levels: bad entity counts");
    LK_REQUIRE(depth && (n == 0 || (users && items && level)),
               "lk_funksvd_plan_levels: null pointer");
    // the level of each entity's latest sample; levels count from 1 here, 0 = no sample yet
    std::vector<int32_t> last_u((size_t)n_users, 0), last_i((size_t)n_items, 0);
    int32_t deepest = 0;
    for (int64_t s = 0; s < n; ++s) {
        const int32_t u = users[s], i = items[s];
        LK_REQUIRE(u >= 0 && u < n_users && i >= 0 && i < n_items,
                   "lk_funksvd_plan_levels: sample %lld is (%d, %d), outside %lld x %lld",
                   (long long)s, u, i, (long long)n_users, (long long)n_items);
        const int32_t a = last_u[u], b = last_i[i];
        const int32_t l = (a > b ? a : b) + 1;
        last_u[u] = l;
        last_i[i] = l;
        level[s] = l - 1;
        if (l > deepest) deepest = l;
    }
    *depth = deepest;
    return LK_OK;
}

extern "C" int lk_funksvd_plan_order(const int32_t *level, int64_t n, int32_t depth,
                                     int64_t *order, int64_t *level_ptr, int32_t *run_end)
{
    LK_REQUIRE(n >= 0 && depth >= 0, "lk_funksvd_plan_order: negative size");
    LK_REQUIRE(level_ptr && (n == 0 || (level && order)) && (depth == 0 || run_end),
               "lk_funksvd_plan_order: null pointer");
    for (int32_t l = 0; l <= depth; ++l) level_ptr[l] = 0;
    for (int64_t s = 0; s < n; ++s) {
        LK_REQUIRE(level[s] >= 0 && level[s] < depth,
                   "lk_funksvd_plan_order: level[%lld] = %d outside 0..%d", (long long)s, level[s],
                   depth);
        ++level_ptr[level[s] + 1];
    }
    for (int32_t l = 0; l < depth; ++l) level_ptr[l + 1] += level_ptr[l];
    std::vector<int64_t> next(level_ptr, level_ptr + depth);
    for (int64_t s = 0; s < n; ++s) order[next[level[s]]++] = s;  // stable: ascending s in a level
    // run_end[l]: one past the last level of the narrow run that holds l; l itself for a wide one.
    // A run is extended level by level while the levels are narrow and it holds <= STAGE samples.
    for (int32_t l = 0; l < depth;) {
        if (level_ptr[l + 1] - level_ptr[l] > lk::funksvd::NARROW) {
            run_end[l] = l;
            ++l;
            continue;
        }
        int32_t e = l + 1;
        while (e < depth && level_ptr[e + 1] - level_ptr[e] <= lk::funksvd::NARROW &&
               level_ptr[e + 1] - level_ptr[l] <= lk::funksvd::STAGE)
            ++e;
        for (; l < e; ++l) run_end[l] = e;
    }
    return LK_OK;
}

extern "C" int lk_funksvd_train_feature(const int32_t *d_users, const int32_t *d_items,
                                        const float *d_ratings, float *d_est,
                                        const int64_t *d_level_ptr, const int32_t *d_run_end,
                                        int32_t depth, float *d_ucol, float *d_icol,
                                        int64_t n_users, int64_t n_items, int32_t epochs,
                                        int32_t finish, double lr, double reg, double trail,
                                        double rmin, double rmax, int32_t flags, double *d_sse,
                                        void *stream)
{
    using namespace lk::funksvd;
    LK_REQUIRE(depth >= 0 && epochs >= 0, "lk_funksvd_train_feature: negative depth or epochs");
    LK_REQUIRE(n_users >= 0 && n_items >= 0 && n_users < ((int64_t)1 << 31) &&
                   n_items < ((int64_t)1 << 31),
               "lk_funksvd_train_feature: bad entity counts");
    LK_REQUIRE(d_level_ptr, "lk_funksvd_train_feature: null level_ptr");
    LK_REQUIRE(depth == 0 || (d_users && d_items && d_ratings && d_est && d_run_end && d_ucol &&
                              d_icol),
               "lk_funksvd_train_feature: null pointer");
    LK_REQUIRE(epochs == 0 || d_sse, "lk_funksvd_train_feature: null sse");
    LK_REQUIRE(!(rmin > rmax), "lk_funksvd_train_feature: rmin > rmax");
    LK_REQUIRE((flags & ~LK_FUNKSVD_GLOBAL_COLUMNS) == 0,
               "lk_funksvd_train_feature: unknown flags %d", flags);
    if (depth == 0 || (epochs == 0 && !finish)) return LK_OK;
    hipStream_t st = lk::as_stream(stream);
    const bool in_lds = !(flags & LK_FUNKSVD_GLOBAL_COLUMNS) &&
                        ((size_t)n_users + (size_t)n_items) * sizeof(float) <= LDS_COLUMN_BYTES;
    if (in_lds)
        return launch<true>(d_users, d_items, d_ratings, d_est, d_level_ptr, d_run_end, depth,
                            d_ucol, d_icol, (int32_t)n_users, (int32_t)n_items, epochs, finish, lr,
                            reg, trail, rmin, rmax, d_sse, st);
    return launch<false>(d_users, d_items, d_ratings, d_est, d_level_ptr, d_run_end, depth, d_ucol,
                         d_icol, (int32_t)n_users, (int32_t)n_items, epochs, finish, lr, reg,
                         trail, rmin, rmax, d_sse, st);
}
