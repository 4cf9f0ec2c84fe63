// als_plan.hip -- the ALS plan object (als_plan.h): its construction, queries and settings, the
// dispatch of a half-epoch to the solver families (als_chol.hip: padded k <= 64, als_blk.hip:
// 128 / 256, als_big.hip: above 256, als_cg.hip: the CG option), the status read and the
// host-buffer entries.  Host code but for the key read of lk_als_plan_order_units: every kernel of
// a half-epoch is launched from the family's own file.
//
// Which kernel takes which task range is decided here, once, when the plan is created: the
// switches that choose them (LK_ALS_WB*, LK_ALS_SIDE_STREAM, LK_BLK_CHUNK_DMA, LK_ALS_CG_HYBRID;
// INTEGRATION.md) are read by plan creation and the launchers read the plan's fields.
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "als_plan.h"
#include "common.h"

namespace lk {

// the plan's rhs side stream (als_plan.h): created on first use, returned by lk_als_plan_destroy
int plan_fork_rhs(const lk_als_plan *p, hipStream_t st, hipStream_t *side)
{
    *side = st;
    if (!p->side_streams) return LK_OK;
    if (!p->side_rhs) {
        p->side_rhs = lk::side_stream_acquire();
        LK_REQUIRE(p->side_rhs != nullptr, "als: no side stream");
        LK_HIP_CHECK(hipEventCreateWithFlags(&p->ev_fork_rhs, hipEventDisableTiming));
        LK_HIP_CHECK(hipEventCreateWithFlags(&p->ev_join_rhs, hipEventDisableTiming));
        LK_HIP_CHECK(hipEventCreateWithFlags(&p->ev_mid_rhs, hipEventDisableTiming));
        LK_HIP_CHECK(hipEventCreateWithFlags(&p->ev_tail_rhs, hipEventDisableTiming));
    }
    LK_HIP_CHECK(hipEventRecord(p->ev_fork_rhs, st));
    LK_HIP_CHECK(hipStreamWaitEvent(p->side_rhs, p->ev_fork_rhs, 0));
    *side = p->side_rhs;
    return LK_OK;
}

// (no side stream without side_streams: plan_fork_rhs creates it)
int plan_rhs_wait_main(const lk_als_plan *p, hipStream_t st)
{
    if (!p->side_rhs) return LK_OK;
    LK_HIP_CHECK(hipEventRecord(p->ev_mid_rhs, st));
    LK_HIP_CHECK(hipStreamWaitEvent(p->side_rhs, p->ev_mid_rhs, 0));
    return LK_OK;
}

int plan_join_rhs(const lk_als_plan *p, hipStream_t st)
{
    if (!p->side_rhs) return LK_OK;
    LK_HIP_CHECK(hipEventRecord(p->ev_join_rhs, p->side_rhs));
    LK_HIP_CHECK(hipStreamWaitEvent(st, p->ev_join_rhs, 0));
    return LK_OK;
}

}  // namespace lk

extern "C" int32_t lk_padded_dim(int32_t k)
{
    if (k < 1) return 0;
    if (k <= 16) return 16;
    if (k <= 32) return 32;
    if (k <= 64) return 64;
    if (k <= 128) return 128;
    if (k <= 256) return 256;
    // above 256: multiples of 64 up to 1024, served by the HBM-tile solver of als_big.hip
    if (k <= 1024) return (k + 63) / 64 * 64;
    return 0;
}

// ---- pool of schedule buffers (per device; plans of a few thousand rows come and go per call) ----
namespace {
struct PackPool {
    static constexpr int SLOTS = 8;
    static constexpr size_t MAX_BYTES = (size_t)8 << 20;  // larger buffers are not pooled
    std::mutex mu;
    struct Slot {
        char *ptr = nullptr;
        size_t cap = 0;
        int dev = -1;
    } slot[SLOTS];
};
PackPool &pack_pool()
{
    static PackPool pool;
    return pool;
}
char *pack_pool_take(size_t bytes, size_t *cap)
{
    if (bytes > PackPool::MAX_BYTES) return nullptr;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    PackPool &pl = pack_pool();
    std::lock_guard<std::mutex> lock(pl.mu);
    int best = -1;
    for (int i = 0; i < PackPool::SLOTS; ++i)
        if (pl.slot[i].ptr && pl.slot[i].dev == dev && pl.slot[i].cap >= bytes &&
            (best < 0 || pl.slot[i].cap < pl.slot[best].cap))
            best = i;
    if (best < 0) return nullptr;
    char *ptr = pl.slot[best].ptr;
    *cap = pl.slot[best].cap;
    pl.slot[best].ptr = nullptr;
    return ptr;
}
bool pack_pool_give(char *ptr, size_t cap)
{
    if (cap > PackPool::MAX_BYTES) return false;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    PackPool &pl = pack_pool();
    std::lock_guard<std::mutex> lock(pl.mu);
    for (int i = 0; i < PackPool::SLOTS; ++i)
        if (!pl.slot[i].ptr) {
            pl.slot[i].ptr = ptr;
            pl.slot[i].cap = cap;
            pl.slot[i].dev = dev;
            return true;
        }
    return false;  // pool full: the caller frees
}
}  // namespace

// a kernel switch of INTEGRATION.md's table: on unless its variable starts with '0'
static bool switch_on(const char *name)
{
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}

// compute units of a device, 0 if it cannot be asked (asked once per device: fold-in plans are
// built per call)
static int device_cu_count(int dev)
{
    static std::mutex mu;
    static int known[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    const bool slot = dev >= 0 && dev < 64;
    if (slot && known[dev] > 0) return known[dev];
    int n = 0;
    if (dev < 0 ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0)
        n = 0;
    if (slot) known[dev] = n;
    return n;
}

extern "C" int lk_als_plan_create_ex(lk_als_plan **out, const void *h_indptr, int indptr_is_64,
                                     int64_t n_rows, int32_t k, int32_t solver, int32_t flags);

extern "C" int lk_als_plan_create(lk_als_plan **out, const void *h_indptr, int indptr_is_64,
                                  int64_t n_rows, int32_t k, int32_t solver)
{
    // the default is the hybrid order (include/lkamd.h); LK_ALS_RHS_ORDER=accurate: the tuned
    // kernels' own summation on every row (round 4's default)
    // (case-insensitive, unknown values refused -- the rules of lkpy_amd._device.als_order_mode.
    // `reference` = the STRICT mode needs the caller's right-hand-side workspace
    // (lk_als_plan_set_rhs_workspace): a plan made here gets the flag, the caller attaches the
    // buffer; until then its rows > 256 entries sum the normal matrix in the reference's blocks
    // and the right-hand side in the kernels' own order)
    const char *e = getenv("LK_ALS_RHS_ORDER");
    int32_t flags = LK_ALS_PLAN_HYBRID_ORDER;
    if (e && e[0]) {
        if (!strcasecmp(e, "accurate")) flags = 0;
        else if (!strcasecmp(e, "reference")) flags = LK_ALS_PLAN_REFERENCE_ORDER;
        else
            LK_REQUIRE(!strcasecmp(e, "auto") || !strcasecmp(e, "hybrid") || !strcasecmp(e, "default"),
                       "lk_als_plan_create: unknown LK_ALS_RHS_ORDER '%s' (auto / reference / accurate)",
                       e);
    }
    return lk_als_plan_create_ex(out, h_indptr, indptr_is_64, n_rows, k, solver, flags);
}

extern "C" int lk_als_plan_create_ex(lk_als_plan **out, const void *h_indptr, int indptr_is_64,
                                     int64_t n_rows, int32_t k, int32_t solver, int32_t flags)
{
    LK_REQUIRE(out != nullptr && h_indptr != nullptr, "lk_als_plan_create: null pointer");
    LK_REQUIRE((flags & ~(LK_ALS_PLAN_REFERENCE_ORDER | LK_ALS_PLAN_HYBRID_ORDER |
                          LK_ALS_PLAN_BAND_UNITS)) == 0,
               "lk_als_plan_create_ex: unknown flags");
    LK_REQUIRE((flags & (LK_ALS_PLAN_REFERENCE_ORDER | LK_ALS_PLAN_HYBRID_ORDER)) !=
                   (LK_ALS_PLAN_REFERENCE_ORDER | LK_ALS_PLAN_HYBRID_ORDER),
               "lk_als_plan_create_ex: reference order is either strict or hybrid");
    LK_REQUIRE(n_rows >= 0 && n_rows < (int64_t)INT32_MAX, "lk_als_plan_create: bad n_rows");
    int KP = lk_padded_dim(k);
    LK_REQUIRE(KP > 0, "lk_als_plan_create: unsupported embedding size k=%d (1..1024)", k);
    // the reference solves every row exactly (sposv): so does AUTO, at every k
    if (solver == LK_SOLVER_AUTO) solver = LK_SOLVER_CHOLESKY;
    LK_REQUIRE(solver == LK_SOLVER_CHOLESKY || solver == LK_SOLVER_CG,
               "lk_als_plan_create: unknown solver %d", solver);
    LK_REQUIRE(!(solver == LK_SOLVER_CG && (KP < 64 || KP > 256)),
               "lk_als_plan_create: the CG solver serves 32 < k <= 256 (got %d)", k);
    LK_REQUIRE(!((flags & LK_ALS_PLAN_REFERENCE_ORDER) && KP > 256),
               "lk_als_plan_create_ex: reference-order plans stop at k = 256 (got %d)", k);

    auto *p = new lk_als_plan();
    p->n_rows = n_rows;
    p->k = k;
    p->KP = KP;
    p->NT = KP / 16;
    p->solver = solver;
    p->is64 = indptr_is_64 ? 1 : 0;
    p->cg_max_iter = 0;
    (void)hipGetDevice(&p->device);
    if (flags & LK_ALS_PLAN_REFERENCE_ORDER) {
        if (solver != LK_SOLVER_CHOLESKY) {
            delete p;
            lk::set_error("lk_als_plan_create_ex: reference order belongs to the exact solver");
            return LK_E_INVALID;
        }
        p->ref_order = true;
        p->chunk = 256;     // matrixmultiply's KC (oracle/lk_oracle.c: LKO_SGEMM_KC)
        p->long_row = 256;  // every row the reference sums in more than one block
    }
    if ((flags & LK_ALS_PLAN_HYBRID_ORDER) && solver == LK_SOLVER_CHOLESKY && KP <= 256) {
        // (the CG option and k > 256 have no slab path: the flag does not apply to them)
        p->hybrid = true;
        p->chunk = 256;
        const char *e = getenv("LK_ALS_REF_LEN");
        int rl = e ? atoi(e) : LK_ALS_LONG_ROW;
        if (rl < 256) rl = 256;                          // (one block: nothing to reorder)
        if (rl > LK_ALS_LONG_ROW) rl = LK_ALS_LONG_ROW;  // longer rows must be chunked anyway
        p->long_row = rl;
    }
    // (k > 256: no chunk slabs -- als_big.hip spreads a long row over its Gram grid)
    const int64_t CHUNK = p->chunk, LONG_ROW = KP > 256 ? INT64_MAX : (int64_t)p->long_row;

    auto len = [&](int64_t r) -> int64_t {
        if (indptr_is_64) {
            const int64_t *ip = static_cast<const int64_t *>(h_indptr);
            return ip[r + 1] - ip[r];
        }
        const int32_t *ip = static_cast<const int32_t *>(h_indptr);
        return (int64_t)ip[r + 1] - ip[r];
    };
    auto start = [&](int64_t r) -> int64_t {
        return indptr_is_64 ? static_cast<const int64_t *>(h_indptr)[r]
                            : (int64_t) static_cast<const int32_t *>(h_indptr)[r];
    };

    // rows by descending length, ties in row order.  Lengths are small integers: a counting sort
    // (histogram of the lengths, offsets from the longest down, rows placed in row order) does in
    // O(rows + longest) what the stable comparison sort did in O(rows log rows) -- a fold-in plan
    // is built per call (10 000 rows: 0.3 of the call's 3.3 ms went into the sort), cfg5's user
    // plan orders 10^7 rows.  Only a matrix whose longest row dwarfs its row count sorts keys.
    std::vector<int32_t> order((size_t)n_rows);
    {
        int64_t longest = 0;
        bool sane = true;
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t n = len(r);
            if (n < 0) sane = false;
            if (n > longest) longest = n;
        }
        if (sane && longest <= 4 * n_rows + 65536) {
            std::vector<int64_t> at((size_t)longest + 2, 0);
            for (int64_t r = 0; r < n_rows; ++r) ++at[(size_t)len(r)];
            int64_t run = 0;  // at[n] = first position of the rows of length n (longest first)
            for (int64_t n = longest; n >= 0; --n) {
                const int64_t c = at[(size_t)n];
                at[(size_t)n] = run;
                run += c;
            }
            for (int64_t r = 0; r < n_rows; ++r) order[(size_t)(at[(size_t)len(r)]++)] = (int32_t)r;
        } else {
            for (int64_t r = 0; r < n_rows; ++r) order[(size_t)r] = (int32_t)r;
            std::stable_sort(order.begin(), order.end(),
                             [&](int32_t x, int32_t y) { return len(x) > len(y); });
        }
    }

    // first task in [lo, hi) of the longest-first order whose row has at most n entries
    auto first_at_most = [&](int64_t n, int64_t lo, int64_t hi) -> int64_t {
        return std::partition_point(order.begin() + lo, order.begin() + hi,
                                    [&](int32_t r) { return len(r) > n; }) -
               order.begin();
    };
    p->t_short = first_at_most(16, 0, n_rows);
    const int64_t t_8 = first_at_most(8, p->t_short, n_rows);
    const int64_t t_4 = first_at_most(4, t_8, n_rows);
    const int64_t t_64 = first_at_most(64, 0, p->t_short);
    const int64_t t_32 = first_at_most(32, t_64, p->t_short);
    const int64_t t_128 = first_at_most(128, 0, t_64);
    // rows [t_cg, n_rows) have at most 16384 / KP entries (256 / 128 / 64 at padded k = 64 /
    // 128 / 256): what the CG kernel keeps in registers over its iterations (als_cg.hip)
    const int64_t cg_len = 16384 / KP;
    const int64_t t_cg = first_at_most(cg_len, 0, n_rows);
    p->t_cg1 = first_at_most(cg_len / 4, t_cg, n_rows);  // ... and that ONE wave holds

    // the Woodbury ranges (als_plan.h).  LK_ALS_WB4=0 / LK_ALS_WB8=0: rows with <= 4 / 5 .. 8
    // entries take the wave-per-row kernel; LK_ALS_WB64=0: rows with 17 .. 64 entries stay on the
    // dense kernel, and so do those with 65 .. 128 (LK_ALS_WB128=0: only these)
    p->t_wb4 = switch_on("LK_ALS_WB4") ? t_4 : n_rows;
    p->t_wb8 = switch_on("LK_ALS_WB8") ? t_8 : p->t_wb4;
    const char *e_k128 = getenv("LK_ALS_WB64_K128");
    const int k128 = e_k128 ? atoi(e_k128) : LK_ALS_WB64_K128_DEFAULT;
    // (17 .. 64 entries: only at padded k = 256 by default -- at k = 128 the 64 x 64 system costs
    // as much as the dense solve of als_blk.hip, measured on the ML-25M shape)
    const int64_t t_wb = (KP == 256 || k128 >= 64) ? t_64 : (k128 >= 32 ? t_32 : p->t_short);
    p->wb_rows = n_rows - t_wb;
    const bool wb64 = switch_on("LK_ALS_WB64");
    p->t_wb64 = wb64 ? t_wb : p->t_short;
    const bool wb128 = KP == 256 && wb64 && switch_on("LK_ALS_WB128") && t_128 < t_64;
    p->t_wb128 = wb128 ? t_128 : p->t_wb64;
    // LK_ALS_SIDE_STREAM=0: OtOr^-1 and the right-hand-side chains on the launch stream
    p->side_streams = switch_on("LK_ALS_SIDE_STREAM");
    // LK_BLK_CHUNK_DMA=0: the register-ring chunk kernel at k = 256 too
    p->chunk_dma = KP == 256 && switch_on("LK_BLK_CHUNK_DMA");

    std::vector<int32_t> row_slab((size_t)n_rows, -1);
    std::vector<int32_t> chunk_row, chunk_slab;
    std::vector<int64_t> chunk_beg;
    std::vector<int32_t> chunk_len;
    // work units (als_plan.h): hybrid plans at padded k = 64 run units of 1024, 512 or 256 entries,
    // one slab per 256-entry block (LK_ALS_REF_UNIT: entries per unit, a multiple of 256; 256 = a
    // unit per block)
    p->unit = p->chunk;
    // (padded k = 256: the LDS-staged chunk kernel of als_blk.hip takes units as well; the
    // register-ring kernel -- no chunk_dma -- has no block boundaries: a unit is a chunk)
    // (padded k = 64: the LDS-DMA Gram accumulation flushes a slab per 256-entry block)
    if (p->hybrid && (KP == 64 || p->chunk_dma)) {
        const char *e = getenv("LK_ALS_REF_UNIT");
        int u = e ? atoi(e) : LK_ALS_CHUNK;
        // LK_ALS_PLAN_BAND_UNITS: the caller orders the units band by band
        // (lk_als_plan_order_units) -- a unit per block keeps the bands tightest and measured
        // fastest; LK_ALS_UNIT_ORDER=0 keeps today's rule with today's order
        if (!e && KP == 64 && (flags & LK_ALS_PLAN_BAND_UNITS) && switch_on("LK_ALS_UNIT_ORDER"))
            u = p->chunk;
        else if (!e && KP == 64) {
            // als_chunk_kernel runs one wave per unit: the largest unit of 1024 / 512 / 256 entries
            // that still gives every chunk wave the device holds two units (a plan with fewer
            // long-row entries than that fills the machine only with a unit per block: ML-25M's
            // user side, 5 310 blocks in 1 507 units of 1024, ran one or two waves per SIMD)
            const int cus = device_cu_count(p->device);
            if (cus <= 0) {
                delete p;
                lk::set_error("lk_als_plan_create: cannot read the device's compute-unit count");
                return LK_E_HIP;
            }
            const int64_t want = 2 * (int64_t)cus * lk::als_chol_chunk_wgs_per_cu() * 4;
            int64_t units_1024 = 0, units_512 = 0;
            for (int64_t r = 0; r < n_rows; ++r) {
                const int64_t n = len(r);
                if (n > LONG_ROW) {
                    units_1024 += (n + 1023) / 1024;
                    units_512 += (n + 511) / 512;
                }
            }
            u = units_1024 >= want ? 1024 : (units_512 >= want ? 512 : 256);
        }
        if (u < p->chunk) u = p->chunk;
        p->unit = u / p->chunk * p->chunk;
    }
    const int64_t UNIT = p->unit;
    {  // (CG plans too: their chunked rows are solved by the exact kernels, als_cg.hip)
        for (int64_t r = 0; r < n_rows; ++r) {
            int64_t n = len(r);
            if (n > LONG_ROW) {
                row_slab[(size_t)r] = (int32_t)p->n_slabs;
                for (int64_t o = 0; o < n; o += UNIT) {
                    chunk_row.push_back((int32_t)r);
                    chunk_beg.push_back(start(r) + o);
                    chunk_len.push_back((int32_t)std::min<int64_t>(UNIT, n - o));
                    chunk_slab.push_back((int32_t)(p->n_slabs + o / CHUNK));
                }
                p->n_slabs += (n + CHUNK - 1) / CHUNK;
                p->n_long++;
            }
        }
    }
    if (p->n_slabs >= (int64_t)INT32_MAX) {
        delete p;
        lk::set_error("lk_als_plan_create: too many slabs");
        return LK_E_INVALID;
    }
    p->n_chunks = (int64_t)chunk_row.size();
    // LK_ALS_CG_HYBRID (CG plans): 0 = CG for every row; 1 = the chunked rows (more than
    // LK_ALS_LONG_ROW entries) go to the exact kernels; default 2 = every row longer than the CG
    // kernel keeps in registers does
    const char *e_cg = getenv("LK_ALS_CG_HYBRID");
    const int cg_mode = (e_cg && e_cg[0] >= '0' && e_cg[0] <= '2') ? e_cg[0] - '0' : 2;
    p->cg_exact = cg_mode == 2 ? t_cg : (cg_mode == 1 ? p->n_long : 0);
    // slab groups of the rows with many chunks (LK_ALS_SLAB_GROUP, als_plan.h)
    std::vector<int32_t> grp_head, grp_cnt;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (row_slab[(size_t)r] < 0) continue;
        const int64_t ns = (len(r) + CHUNK - 1) / CHUNK;
        if (p->ref_order || p->hybrid) {  // ONE group per row: head += every other slab, in chunk order
            grp_head.push_back(row_slab[(size_t)r]);
            grp_cnt.push_back((int32_t)ns);
            continue;
        }
        if (ns <= LK_ALS_SLAB_GROUP) continue;
        for (int64_t s0 = 0; s0 < ns; s0 += LK_ALS_SLAB_GROUP) {
            const int64_t c = std::min<int64_t>(LK_ALS_SLAB_GROUP, ns - s0);
            if (c >= 2) {
                grp_head.push_back((int32_t)(row_slab[(size_t)r] + s0));
                grp_cnt.push_back((int32_t)c);
            }
        }
    }
    p->n_groups = (int64_t)grp_head.size();

    // the schedule arrays: ONE device allocation and ONE copy (a fold-in plan of a batch of queries
    // is built per call -- eight allocations and blocking copies were 0.4 ms of a 4 ms call)
    {
        auto padded = [](size_t bytes) { return lk::align_up(std::max<size_t>(bytes, 8), 256); };
        const size_t b_order = padded(order.size() * 4), b_rslab = padded(row_slab.size() * 4),
                     b_crow = padded(chunk_row.size() * 4), b_cbeg = padded(chunk_beg.size() * 8),
                     b_cslab = padded(chunk_slab.size() * 4), b_ghead = padded(grp_head.size() * 4),
                     b_gcnt = padded(grp_cnt.size() * 4), b_clen = padded(chunk_len.size() * 4);
        const size_t total = b_order + b_rslab + b_crow + b_cbeg + b_cslab + b_ghead + b_gcnt + b_clen;
        std::vector<char> host(total, 0);
        size_t o = 0;
        auto put = [&](const void *src, size_t bytes, size_t slot) {
            if (bytes) memcpy(host.data() + o, src, bytes);
            const size_t at = o;
            o += slot;
            return at;
        };
        const size_t o_order = put(order.data(), order.size() * 4, b_order);
        const size_t o_rslab = put(row_slab.data(), row_slab.size() * 4, b_rslab);
        const size_t o_cbeg = put(chunk_beg.data(), chunk_beg.size() * 8, b_cbeg);
        const size_t o_crow = put(chunk_row.data(), chunk_row.size() * 4, b_crow);
        const size_t o_cslab = put(chunk_slab.data(), chunk_slab.size() * 4, b_cslab);
        const size_t o_ghead = put(grp_head.data(), grp_head.size() * 4, b_ghead);
        const size_t o_gcnt = put(grp_cnt.data(), grp_cnt.size() * 4, b_gcnt);
        const size_t o_clen = put(chunk_len.data(), chunk_len.size() * 4, b_clen);
        hipError_t e = hipSuccess;
        p->d_pack = pack_pool_take(total, &p->pack_cap);
        if (!p->d_pack) {
            p->pack_cap = total;
            e = hipMalloc(reinterpret_cast<void **>(&p->d_pack), total);
        }
        if (e == hipSuccess) e = hipMemcpy(p->d_pack, host.data(), total, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            lk::set_error("lk_als_plan_create: %s", hipGetErrorString(e));
            lk_als_plan_destroy(p);
            return LK_E_HIP;
        }
        p->d_order = reinterpret_cast<int32_t *>(p->d_pack + o_order);
        p->d_row_slab = reinterpret_cast<int32_t *>(p->d_pack + o_rslab);
        p->d_chunk_beg = reinterpret_cast<int64_t *>(p->d_pack + o_cbeg);
        p->d_chunk_row = reinterpret_cast<int32_t *>(p->d_pack + o_crow);
        p->d_chunk_slab = reinterpret_cast<int32_t *>(p->d_pack + o_cslab);
        p->d_grp_head = reinterpret_cast<int32_t *>(p->d_pack + o_ghead);
        p->d_grp_cnt = reinterpret_cast<int32_t *>(p->d_pack + o_gcnt);
        p->d_chunk_len = reinterpret_cast<int32_t *>(p->d_pack + o_clen);
    }

    size_t off = 0;
    p->off_status = off;
    off += 256;
    p->off_otor = off;
    off += lk::align_up((size_t)KP * KP * sizeof(float), 256);
    p->off_delta = off;
    off += lk::align_up((size_t)std::max<int64_t>(n_rows, 1) * sizeof(float), 256);
    p->off_partial = off;
    off += lk::align_up((size_t)LK_DELTA_BLOCKS * sizeof(float), 256);
    p->off_slabs = off;
    // one-wave slabs (als_chol.hip, k <= 64) or four-wave slabs (als_blk.hip, k = 128 / 256)
    if (KP > 256) {
        // the tile scratch of a batch of rows (als_big.hip) takes the slabs' place
        off += lk::align_up(lk::als_big_scratch_bytes(KP, n_rows), 256);
    } else {
        size_t slab_f = KP > 64 ? lk::als_blk_slab_floats(p->NT) : lk::als_chol_slab_floats(p->NT);
        off += lk::align_up((size_t)std::max<int64_t>(p->n_slabs, 1) * slab_f * sizeof(float),
                            256);
    }
    if (p->hybrid) {  // y of the long rows in the reference's order, one row of KP floats per task
        p->off_yref = off;
        off += lk::align_up((size_t)std::max<int64_t>(p->n_long, 1) * KP * sizeof(float), 256);
    }
    if (KP > 64 && KP <= 256) {  // OtOr^-1 for the Woodbury rows (lk_als_plan_set_z_workspace)
        p->off_ginv = off;
        off += lk::align_up((size_t)KP * KP * sizeof(float), 256);
        p->off_invws = off;
        off += lk::align_up(lk::spd_inverse_workspace_bytes(KP), 256);
    }
    p->ws_bytes = off;
    *out = p;
    return LK_OK;
}

extern "C" int lk_als_plan_enable_timing(lk_als_plan *p, int enable)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_enable_timing: null plan");
    if (enable && !p->ev[0][0]) {
        for (int i = 0; i < lk_als_plan::TIMING_RING; ++i)
            for (int j = 0; j < 3; ++j) LK_HIP_CHECK(hipEventCreate(&p->ev[i][j]));
    }
    p->timing = enable != 0;
    p->timing_n = 0;
    return LK_OK;
}

extern "C" int lk_als_plan_get_timing(lk_als_plan *p, double *ms_chunk, double *ms_solve,
                                      int32_t *n_launches)
{
    LK_REQUIRE(p && ms_chunk && ms_solve && n_launches, "lk_als_plan_get_timing: null pointer");
    *ms_chunk = 0.0;
    *ms_solve = 0.0;
    *n_launches = p->timing_n;
    for (int i = 0; i < p->timing_n; ++i) {
        float a = 0.f, b = 0.f;
        LK_HIP_CHECK(hipEventSynchronize(p->ev[i][2]));
        LK_HIP_CHECK(hipEventElapsedTime(&a, p->ev[i][0], p->ev[i][1]));
        LK_HIP_CHECK(hipEventElapsedTime(&b, p->ev[i][1], p->ev[i][2]));
        *ms_chunk += a;
        *ms_solve += b;
    }
    p->timing_n = 0;
    return LK_OK;
}

extern "C" void lk_als_plan_destroy(lk_als_plan *p)
{
    if (!p) return;
    // the plan's device is current for the call (the synchronisation below waits for it, its
    // schedule buffer and side streams go back to ITS pools), the caller's again afterwards
    int caller = -1;
    const bool swap = p->device >= 0 && hipGetDevice(&caller) == hipSuccess &&
                      caller != p->device && hipSetDevice(p->device) == hipSuccess;
    if (p->ev[0][0])
        for (int i = 0; i < lk_als_plan::TIMING_RING; ++i)
            for (int j = 0; j < 3; ++j) (void)hipEventDestroy(p->ev[i][j]);
    if (p->side) {
        (void)hipStreamSynchronize(p->side);
        lk::side_stream_release(p->side);
        (void)hipEventDestroy(p->ev_fork);
        (void)hipEventDestroy(p->ev_join);
    }
    if (p->side_rhs) {
        (void)hipStreamSynchronize(p->side_rhs);
        lk::side_stream_release(p->side_rhs);
        (void)hipEventDestroy(p->ev_fork_rhs);
        (void)hipEventDestroy(p->ev_join_rhs);
        (void)hipEventDestroy(p->ev_mid_rhs);
        (void)hipEventDestroy(p->ev_tail_rhs);
    }
    // (d_order ... d_chunk_len point into d_pack.)  Small schedule buffers go back to a per-device
    // pool instead of hipFree: a fold-in plan lives for one call, and hipMalloc + hipFree were a
    // quarter of a millisecond of it.  hipFree waits for the device; so does this.
    if (p->d_pack) {
        (void)hipDeviceSynchronize();
        if (!pack_pool_give(p->d_pack, p->pack_cap)) (void)hipFree(p->d_pack);
    }
    if (swap) (void)hipSetDevice(caller);
    delete p;
}

extern "C" size_t lk_als_plan_workspace_bytes(const lk_als_plan *p) { return p ? p->ws_bytes : 0; }
extern "C" int32_t lk_als_plan_solver(const lk_als_plan *p) { return p ? p->solver : -1; }

extern "C" int lk_als_plan_set_ctl(lk_als_plan *p, lk_task_ctl *ctl)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_ctl: null plan");
    p->ctl = ctl;
    return LK_OK;
}

extern "C" int64_t lk_als_plan_short_rows(const lk_als_plan *p)
{
    return p ? p->n_rows - p->t_short : 0;
}

extern "C" int64_t lk_als_plan_long_rows(const lk_als_plan *p) { return p ? p->n_long : 0; }
extern "C" int64_t lk_als_plan_units(const lk_als_plan *p) { return p ? p->n_chunks : 0; }
extern "C" int32_t lk_als_plan_unit(const lk_als_plan *p) { return p ? p->unit : 0; }

// ---- the order of the work units ----
namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes)
    {
        LK_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
        return LK_OK;
    }
};

// keys[u] = the band unit u starts in: its first column, through col_key where the map covers it
__global__ __launch_bounds__(256) void unit_key_kernel(const int32_t *__restrict__ indices,
                                                       const int64_t *__restrict__ chunk_beg,
                                                       int64_t n_units,
                                                       const int32_t *__restrict__ col_key,
                                                       int64_t n_col_key, int32_t *__restrict__ keys)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_units) return;
    const int32_t c = indices[chunk_beg[u]];  // (a unit has at least one entry)
    keys[u] = (col_key && c >= 0 && c < n_col_key) ? col_key[c] : c;
}
}  // namespace

extern "C" int lk_als_plan_order_units(lk_als_plan *p, const int32_t *d_indices,
                                       const int32_t *d_col_key, int64_t n_col_key, void *stream)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_order_units: null plan");
    // (padded k > 64: als_blk.hip's register-ring launch takes slab = unit, in table order)
    if (p->n_chunks == 0 || p->KP > 64 || !switch_on("LK_ALS_UNIT_ORDER")) return LK_OK;
    LK_REQUIRE(d_indices != nullptr, "lk_als_plan_order_units: null indices");
    LK_REQUIRE(d_col_key == nullptr || n_col_key > 0, "lk_als_plan_order_units: empty key map");
    hipStream_t st = lk::as_stream(stream);
    const size_t n = (size_t)p->n_chunks;
    // no launch of the plan may read the table while it is rewritten (side streams included)
    LK_HIP_CHECK(hipDeviceSynchronize());
    DevBuf d_keys;
    int rc = d_keys.alloc(n * sizeof(int32_t));
    if (rc != LK_OK) return rc;
    hipLaunchKernelGGL(unit_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       d_indices, p->d_chunk_beg, (int64_t)n, d_col_key, n_col_key,
                       static_cast<int32_t *>(d_keys.p));
    LK_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> key(n), row(n), len(n), slab(n);
    std::vector<int64_t> beg(n);
    LK_HIP_CHECK(hipMemcpyAsync(key.data(), d_keys.p, n * 4, hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipMemcpyAsync(row.data(), p->d_chunk_row, n * 4, hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipMemcpyAsync(len.data(), p->d_chunk_len, n * 4, hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipMemcpyAsync(slab.data(), p->d_chunk_slab, n * 4, hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipMemcpyAsync(beg.data(), p->d_chunk_beg, n * 8, hipMemcpyDeviceToHost, st));
    LK_HIP_CHECK(hipStreamSynchronize(st));
    // (key, row, offset): a total order of the units, whatever order the table is in now -- a
    // second call sorts the same list
    std::vector<int64_t> sorted(n);
    for (size_t u = 0; u < n; ++u) sorted[u] = (int64_t)u;
    std::sort(sorted.begin(), sorted.end(), [&](int64_t a, int64_t b) {
        if (key[a] != key[b]) return key[a] < key[b];
        if (row[a] != row[b]) return row[a] < row[b];
        return beg[a] < beg[b];
    });
    // XCD x receives the physical workgroups b = x, x + 8, ...: they take the next units of the
    // sorted list, four each; the physically last workgroup, wherever it falls, takes what is
    // left of four
    const int64_t n_wg = ((int64_t)n + 3) / 4;
    std::vector<int32_t> o_row(n), o_len(n), o_slab(n);
    std::vector<int64_t> o_beg(n);
    size_t next = 0;
    for (int64_t x = 0; x < (int64_t)lk::XCD_COUNT; ++x)
        for (int64_t b = x; b < n_wg; b += lk::XCD_COUNT)
            for (size_t at = (size_t)b * 4; at < std::min<size_t>((size_t)b * 4 + 4, n); ++at) {
                const size_t u = (size_t)sorted[next++];
                o_row[at] = row[u];
                o_len[at] = len[u];
                o_slab[at] = slab[u];
                o_beg[at] = beg[u];
            }
    LK_HIP_CHECK(hipMemcpyAsync(p->d_chunk_row, o_row.data(), n * 4, hipMemcpyHostToDevice, st));
    LK_HIP_CHECK(hipMemcpyAsync(p->d_chunk_len, o_len.data(), n * 4, hipMemcpyHostToDevice, st));
    LK_HIP_CHECK(hipMemcpyAsync(p->d_chunk_slab, o_slab.data(), n * 4, hipMemcpyHostToDevice, st));
    LK_HIP_CHECK(hipMemcpyAsync(p->d_chunk_beg, o_beg.data(), n * 8, hipMemcpyHostToDevice, st));
    // (the half-epochs may run on other streams than `st`, and the host arrays end here)
    LK_HIP_CHECK(hipDeviceSynchronize());
    return LK_OK;
}

extern "C" int lk_als_plan_unit_table(const lk_als_plan *p, int64_t *out_beg, int32_t *out_len,
                                      int32_t *out_slab)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_unit_table: null plan");
    const size_t n = (size_t)p->n_chunks;
    if (n == 0) return LK_OK;
    LK_HIP_CHECK(hipDeviceSynchronize());
    if (out_beg) LK_HIP_CHECK(hipMemcpy(out_beg, p->d_chunk_beg, n * 8, hipMemcpyDeviceToHost));
    if (out_len) LK_HIP_CHECK(hipMemcpy(out_len, p->d_chunk_len, n * 4, hipMemcpyDeviceToHost));
    if (out_slab) LK_HIP_CHECK(hipMemcpy(out_slab, p->d_chunk_slab, n * 4, hipMemcpyDeviceToHost));
    return LK_OK;
}

extern "C" const float *lk_als_plan_yref(const lk_als_plan *p, const void *d_ws)
{
    if (!p || !d_ws || !p->hybrid) return nullptr;
    return reinterpret_cast<const float *>(static_cast<const char *>(d_ws) + p->off_yref);
}

extern "C" int64_t lk_als_plan_woodbury_rows(const lk_als_plan *p) { return p ? p->wb_rows : 0; }

extern "C" int lk_als_plan_set_z(lk_als_plan *p, const float *d_z)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_z: null plan");
    p->d_z = d_z;
    return LK_OK;
}

extern "C" int lk_als_plan_set_z_shared(lk_als_plan *p, const float *d_z, const void *d_flag)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_z_shared: null plan");
    LK_REQUIRE((d_z == nullptr) == (d_flag == nullptr),
               "lk_als_plan_set_z_shared: Z and its flag word go together");
    LK_REQUIRE(d_z == nullptr || (p->KP > 64 && p->KP <= 256),
               "lk_als_plan_set_z_shared: the Woodbury kernels serve padded k = 128 / 256 only");
    p->d_z = d_z;
    p->d_zflag_src = static_cast<const int *>(d_flag);
    if (d_z) p->d_zbuf = nullptr;
    return LK_OK;
}

extern "C" int lk_als_plan_set_z_leader(lk_als_plan *p, int on)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_z_leader: null plan");
    p->z_for_others = on != 0;
    return LK_OK;
}

extern "C" const void *lk_als_plan_z_flag(const lk_als_plan *p, const void *d_ws)
{
    if (!p || !d_ws) return nullptr;
    return static_cast<const char *>(d_ws) + p->off_status + sizeof(int);
}

extern "C" int lk_als_plan_set_z_workspace(lk_als_plan *p, float *d_zbuf)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_z_workspace: null plan");
    LK_REQUIRE(d_zbuf == nullptr || (p->KP > 64 && p->KP <= 256),
               "lk_als_plan_set_z_workspace: the Woodbury kernels serve padded k = 128 / 256 only");
    p->d_zbuf = d_zbuf;
    if (d_zbuf) {
        p->d_z = nullptr;
        p->d_zflag_src = nullptr;
    }
    return LK_OK;
}

extern "C" int lk_als_plan_set_cg(lk_als_plan *p, float tol, int32_t max_iter)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_cg: null plan");
    LK_REQUIRE(tol > 0.f, "lk_als_plan_set_cg: tol must be positive");
    p->cg_tol = tol;
    p->cg_max_iter = max_iter;
    return LK_OK;
}

extern "C" int lk_als_plan_set_rhs_workspace(lk_als_plan *p, float *d_y)
{
    LK_REQUIRE(p != nullptr, "lk_als_plan_set_rhs_workspace: null plan");
    LK_REQUIRE(d_y == nullptr || p->solver == LK_SOLVER_CHOLESKY,
               "lk_als_plan_set_rhs_workspace: the reference-order right-hand side belongs to the "
               "exact solver (the CG option has no reference to reproduce)");
    p->d_yref = d_y;
    return LK_OK;
}

extern "C" int lk_als_implicit_half_epoch(const lk_als_plan *plan, const void *d_indptr,
                                          const int32_t *d_indices, const float *d_values,
                                          int64_t n_rows, int64_t n_cols, int32_t k,
                                          float *d_this, int32_t ld_this, const float *d_other,
                                          int32_t ld_other, const float *d_otor, int32_t ld_otor,
                                          void *d_ws, float *d_out_frob, void *stream)
{
    LK_REQUIRE(plan != nullptr, "lk_als_implicit_half_epoch: null plan");
    LK_REQUIRE(n_rows == plan->n_rows && k == plan->k,
               "lk_als_implicit_half_epoch: plan built for %lld rows, k=%d; got %lld rows, k=%d",
               (long long)plan->n_rows, plan->k, (long long)n_rows, k);
    LK_REQUIRE(ld_this == plan->KP && ld_other == plan->KP,
               "lk_als_implicit_half_epoch: factor leading dimensions (%d, %d) must equal "
               "lk_padded_dim(k)=%d",
               ld_this, ld_other, plan->KP);
    LK_REQUIRE(ld_otor >= k, "lk_als_implicit_half_epoch: ld_otor < k");
    LK_REQUIRE(d_indptr && d_this && d_otor && d_ws && d_out_frob,
               "lk_als_implicit_half_epoch: null pointer");
    LK_REQUIRE(n_cols >= 0 && (n_cols == 0 || d_other), "lk_als_implicit_half_epoch: null other");
    hipStream_t st = lk::as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    if (plan->solver == LK_SOLVER_CG)
        return lk::als_cg_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows, k,
                                     d_this, ld_this, d_other, ld_other, d_otor, ld_otor, ws,
                                     d_out_frob, st);
    if (plan->KP > 256)
        return lk::als_big_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows, k,
                                      d_this, d_other, d_otor, ld_otor, ws, d_out_frob, st, false,
                                      0.f);
    if (plan->KP > 64)
        return lk::als_blk_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows,
                                      n_cols, k, d_this, d_other, d_otor, ld_otor, ws, d_out_frob,
                                      st, false, 0.f);
    return lk::als_chol_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows, n_cols,
                                   k, d_this, ld_this, d_other, ld_other, d_otor, ld_otor, ws,
                                   d_out_frob, st, false, 0.f);
}

extern "C" int lk_als_implicit_epoch(const lk_als_plan *user_plan, const lk_als_plan *item_plan,
                                     const void *d_u_indptr, const int32_t *d_u_indices,
                                     const float *d_u_values, const void *d_i_indptr,
                                     const int32_t *d_i_indices, const float *d_i_values,
                                     int32_t k, float *d_p, float *d_q, float *d_qtq,
                                     int32_t ld_qtq, float user_reg, float *d_ptp, int32_t ld_ptp,
                                     float item_reg, void *d_user_ws, void *d_item_ws,
                                     void *d_gram_ws, float *d_out_delta, void *stream)
{
    LK_REQUIRE(user_plan && item_plan, "lk_als_implicit_epoch: null plan");
    for (const lk_als_plan *p : {user_plan, item_plan})
        LK_REQUIRE(p->k == k && p->KP <= 64 && p->solver == LK_SOLVER_CHOLESKY && p->hybrid &&
                       !p->ctl && p->dense_limit < 0,
                   "lk_als_implicit_epoch serves hybrid-order plans of the exact solver at padded "
                   "k <= 64 without a task-control block (k=%d here); use the half-epoch calls",
                   k);
    LK_REQUIRE(user_plan != item_plan, "lk_als_implicit_epoch: one plan given twice");
    LK_REQUIRE(ld_qtq >= k && ld_ptp >= k, "lk_als_implicit_epoch: Gramian leading dimension < k");
    LK_REQUIRE(d_u_indptr && d_i_indptr && d_p && d_q && d_qtq && d_ptp && d_user_ws &&
                   d_item_ws && d_gram_ws && d_out_delta,
               "lk_als_implicit_epoch: null pointer");
    LK_REQUIRE(d_user_ws != d_item_ws && d_qtq != d_ptp,
               "lk_als_implicit_epoch: the two halves need buffers of their own");
    return lk::als_chol_epoch(user_plan, item_plan, d_u_indptr, d_u_indices, d_u_values,
                              d_i_indptr, d_i_indices, d_i_values, d_p, d_q, d_qtq, ld_qtq,
                              user_reg, d_ptp, ld_ptp, item_reg, static_cast<char *>(d_user_ws),
                              static_cast<char *>(d_item_ws), static_cast<float *>(d_gram_ws),
                              d_out_delta, lk::as_stream(stream));
}

extern "C" int lk_als_explicit_half_epoch(const lk_als_plan *plan, const void *d_indptr,
                                          const int32_t *d_indices, const float *d_values,
                                          int64_t n_rows, int64_t n_cols, int32_t k,
                                          float *d_this, int32_t ld_this, const float *d_other,
                                          int32_t ld_other, float reg, void *d_ws,
                                          float *d_out_frob, void *stream)
{
    LK_REQUIRE(plan != nullptr, "lk_als_explicit_half_epoch: null plan");
    LK_REQUIRE(n_rows == plan->n_rows && k == plan->k,
               "lk_als_explicit_half_epoch: plan built for %lld rows, k=%d; got %lld rows, k=%d",
               (long long)plan->n_rows, plan->k, (long long)n_rows, k);
    LK_REQUIRE(ld_this == plan->KP && ld_other == plan->KP,
               "lk_als_explicit_half_epoch: factor leading dimensions (%d, %d) must equal "
               "lk_padded_dim(k)=%d",
               ld_this, ld_other, plan->KP);
    LK_REQUIRE(d_indptr && d_this && d_ws && d_out_frob,
               "lk_als_explicit_half_epoch: null pointer");
    LK_REQUIRE(n_cols >= 0 && (n_cols == 0 || d_other), "lk_als_explicit_half_epoch: null other");
    LK_REQUIRE(plan->solver != LK_SOLVER_CG,
               "lk_als_explicit_half_epoch: only the exact (Cholesky) solver is built for the "
               "explicit model");
    hipStream_t st = lk::as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    if (plan->KP > 256)
        return lk::als_big_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows, k,
                                      d_this, d_other, nullptr, 0, ws, d_out_frob, st, true, reg);
    if (plan->KP > 64)
        return lk::als_blk_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows,
                                      n_cols, k, d_this, d_other, nullptr, 0, ws, d_out_frob, st,
                                      true, reg);
    return lk::als_chol_half_epoch(plan, d_indptr, plan->is64, d_indices, d_values, n_rows, n_cols,
                                   k, d_this, ld_this, d_other, ld_other, nullptr, 0, ws,
                                   d_out_frob, st, true, reg);
}

extern "C" int lk_als_check_status(const lk_als_plan *plan, void *d_ws, void *stream)
{
    LK_REQUIRE(plan && d_ws, "lk_als_check_status: null pointer");
    int status[2] = {0, 0};
    LK_HIP_CHECK(hipMemcpyAsync(status, static_cast<char *>(d_ws) + plan->off_status,
                                sizeof(status), hipMemcpyDeviceToHost, lk::as_stream(stream)));
    LK_HIP_CHECK(hipStreamSynchronize(lk::as_stream(stream)));
    if (plan->ctl) {
        // AccelTask protocol: a cancelled task reports the interruption, not a result
        int rc = lk::ctl_finish(plan->ctl, lk::as_stream(stream));
        if (rc != LK_OK) return rc;
    }
    if (status[0] != 0) {
        // reference: RuntimeError("ALS solve error: ...") (src/accel/als/implicit.rs:79)
        lk::set_error("ALS solve error: normal matrix of row %d is not positive definite",
                      status[0] - 1);
        return LK_E_NOT_SPD;
    }
    return LK_OK;
}

extern "C" int lk_als_implicit_half_epoch_host_ctl(const void *h_indptr, int indptr_is_64,
                                                   const int32_t *h_indices,
                                                   const float *h_values, int64_t n_rows,
                                                   int64_t n_cols, int32_t k, float *h_this,
                                                   const float *h_other, const float *h_otor,
                                                   int32_t solver, float *h_out_frob,
                                                   lk_task_ctl *ctl)
{
    LK_REQUIRE(h_indptr && h_this && h_otor && h_out_frob, "half_epoch_host: null pointer");
    LK_REQUIRE(n_rows >= 0 && n_cols >= 0, "half_epoch_host: negative size");
    const int KP = lk_padded_dim(k);
    LK_REQUIRE(KP > 0, "half_epoch_host: unsupported k=%d", k);
    const int64_t nnz = indptr_is_64 ? static_cast<const int64_t *>(h_indptr)[n_rows]
                                     : static_cast<const int32_t *>(h_indptr)[n_rows];
    LK_REQUIRE(nnz >= 0 && (nnz == 0 || (h_indices && h_values && h_other)),
               "half_epoch_host: null pointer");
    lk_als_plan *plan = nullptr;
    int rc = lk_als_plan_create(&plan, h_indptr, indptr_is_64, n_rows, k, solver);
    if (rc != LK_OK) return rc;
    if (ctl && (rc = lk_als_plan_set_ctl(plan, ctl)) != LK_OK) {
        lk_als_plan_destroy(plan);
        return rc;
    }
    const size_t ipb = (size_t)(n_rows + 1) * (indptr_is_64 ? 8 : 4);
    DevBuf ip, idx, val, th, thp, ot, otp, oo, ws, fr, zb;
    auto fail = [&](int c) {
        lk_als_plan_destroy(plan);
        return c;
    };
    if ((rc = ip.alloc(ipb)) || (rc = idx.alloc((size_t)nnz * 4)) ||
        (rc = val.alloc((size_t)nnz * 4)) || (rc = th.alloc((size_t)n_rows * k * 4)) ||
        (rc = thp.alloc((size_t)n_rows * KP * 4)) || (rc = ot.alloc((size_t)n_cols * k * 4)) ||
        (rc = otp.alloc((size_t)n_cols * KP * 4)) || (rc = oo.alloc((size_t)k * k * 4)) ||
        (rc = ws.alloc(lk_als_plan_workspace_bytes(plan))) || (rc = fr.alloc(4)))
        return fail(rc);
    // padded k = 128 / 256, no task control: the short rows take the Woodbury kernels when there
    // are enough of them to pay for Z = other * OtOr^-1 (the rule of lkpy_amd/_device.py::use_woodbury:
    // LK_ALS_WB_MIN_ROWS, default 4096) and no confidence value is negative (they take sqrt(v))
    if (!ctl && KP > 64 && KP <= 256 && plan->solver == LK_SOLVER_CHOLESKY && n_cols > 0) {
        const char *e = getenv("LK_ALS_WB_MIN_ROWS");
        const int64_t wb_min = e ? atoll(e) : 4096;
        bool neg = false;
        for (int64_t i = 0; i < nnz && !neg; ++i) neg = h_values[i] < 0.f;
        if (wb_min > 0 && lk_als_plan_woodbury_rows(plan) >= wb_min && !neg) {
            if ((rc = zb.alloc((size_t)n_cols * KP * 4))) return fail(rc);
            if ((rc = lk_als_plan_set_z_workspace(plan, static_cast<float *>(zb.p)))) return fail(rc);
        }
    }
#define LK_H(expr)                                                              \
    do {                                                                        \
        hipError_t _e = (expr);                                                 \
        if (_e != hipSuccess) {                                                 \
            lk::set_error("%s failed: %s", #expr, hipGetErrorString(_e));       \
            return fail(LK_E_HIP);                                              \
        }                                                                       \
    } while (0)
    LK_H(hipMemcpy(ip.p, h_indptr, ipb, hipMemcpyHostToDevice));
    if (nnz > 0) {
        LK_H(hipMemcpy(idx.p, h_indices, (size_t)nnz * 4, hipMemcpyHostToDevice));
        LK_H(hipMemcpy(val.p, h_values, (size_t)nnz * 4, hipMemcpyHostToDevice));
    }
    if (n_rows > 0) LK_H(hipMemcpy(th.p, h_this, (size_t)n_rows * k * 4, hipMemcpyHostToDevice));
    if (n_cols > 0) LK_H(hipMemcpy(ot.p, h_other, (size_t)n_cols * k * 4, hipMemcpyHostToDevice));
    LK_H(hipMemcpy(oo.p, h_otor, (size_t)k * k * 4, hipMemcpyHostToDevice));
    if ((rc = lk_pad_rows((const float *)th.p, n_rows, k, k, (float *)thp.p, KP, nullptr)) ||
        (rc = lk_pad_rows((const float *)ot.p, n_cols, k, k, (float *)otp.p, KP, nullptr)))
        return fail(rc);
    rc = lk_als_implicit_half_epoch(plan, ip.p, (const int32_t *)idx.p, (const float *)val.p,
                                    n_rows, n_cols, k, (float *)thp.p, KP, (const float *)otp.p,
                                    KP, (const float *)oo.p, k, ws.p, (float *)fr.p, nullptr);
    if (rc != LK_OK) return fail(rc);
    // (LK_E_CANCELLED when the task-control block was cancelled: the rows solved so far are
    // still copied back below -- `this` is updated in place row by row in the reference too)
    const int rc_status = lk_als_check_status(plan, ws.p, nullptr);
    if (rc_status != LK_OK && rc_status != LK_E_CANCELLED) return fail(rc_status);
    // (a failed status leaves the message in lk_last_error: set_error below must not run)
    if ((rc = lk_unpad_rows((const float *)thp.p, n_rows, k, KP, (float *)th.p, k, nullptr)))
        return fail(rc);
    LK_H(hipDeviceSynchronize());
    if (n_rows > 0) LK_H(hipMemcpy(h_this, th.p, (size_t)n_rows * k * 4, hipMemcpyDeviceToHost));
    LK_H(hipMemcpy(h_out_frob, fr.p, 4, hipMemcpyDeviceToHost));
#undef LK_H
    lk_als_plan_destroy(plan);
    return rc_status;
}

extern "C" int lk_als_implicit_half_epoch_host(const void *h_indptr, int indptr_is_64,
                                               const int32_t *h_indices, const float *h_values,
                                               int64_t n_rows, int64_t n_cols, int32_t k,
                                               float *h_this, const float *h_other,
                                               const float *h_otor, int32_t solver,
                                               float *h_out_frob)
{
    return lk_als_implicit_half_epoch_host_ctl(h_indptr, indptr_is_64, h_indices, h_values, n_rows,
                                               n_cols, k, h_this, h_other, h_otor, solver,
                                               h_out_frob, nullptr);
}
