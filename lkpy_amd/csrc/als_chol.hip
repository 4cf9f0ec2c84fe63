// als_chol.hip -- implicit-ALS half-epoch, exact (Cholesky) solver, gfx950.
//
// Stands in for `train_implicit_matrix` / `ImplicitTrainTask::invoke` /
// `train_row_solve` (src/accel/als/implicit.rs:35-125) and `POSV::solve`
// (src/accel/als/solve.rs:65-107).  Per CSR row r with columns c_j, values v_j:
//     A = OtOr + sum_j v_j q_j q_j^T      y = sum_j (v_j + 1) q_j      x = A^-1 y
//     this[r] <- x;   delta_r = ||x - this_old[r]||^2   (empty row: zeros, delta 0)
//
// Work decomposition: ONE WAVE PER ROW (4 independent waves per workgroup, no
// workgroup barriers).  Rows are visited longest-first (plan order); rows longer
// than LK_ALS_LONG_ROW are pre-reduced by a chunk kernel (one wave per chunk of
// <= LK_ALS_CHUNK entries) into partial slabs that the solving wave sums in
// chunk order, so the result is independent of scheduling (bit-reproducible).
//
// Normal-matrix build (the flop carrier, 2*k^2 per CSR entry): f32 MFMA
// v_mfma_f32_16x16x4_f32, K = 4 CSR entries per instruction, upper tiles only
// (A is symmetric): NT(NT+1)/2 MFMAs per 4 entries instead of NT^2.  Features
// are handled in "primed" order p = t*16 + s <-> f = s*NT + t so that a lane's NT
// features of a factor row are one contiguous vector load and 16 lanes fetch the
// whole row of `other` in one coalesced request (the gather is per CSR entry:
// 4*k contiguous bytes).  The CSR (indices, values) stream is read coalesced, 64
// entries per wave-load, and broadcast with ds_bpermute.
//
// Solve: the hybrid Cholesky (below) factors A' (primed order == a symmetric permutation of A,
// which leaves the solution unchanged) in the accumulator tiles: panels of four columns in
// lane = row layout, MFMA updates of the rest; forward substitution rides along, back
// substitution against L^T staged in LDS.
//
// Roofline: f32 MFMA bound for k = 64 (nnz*(2k^2+2k) +
// rows*(k^3/3 + 2k^2) flop per half-epoch); HBM traffic is the CSR stream plus
// the (L2/MALL-resident) gathered factor rows.
#include <algorithm>
#include <utility>

#include "als_plan.h"
#include "common.h"
#include "delta_reduce.h"

#ifndef LK_ALS_RING
#define LK_ALS_RING 4  // gather ring slots (8 costs 20 more registers: no gain at 3 waves/SIMD)
#endif

namespace lk {

#ifdef LK_ALS_PHASES
// Diagnostic build only (tools/als_variants.py): shader-clock cycles per phase of the solve
// kernel, one record of 8 words per task (plan order): [0] row set-up (row id, extents), [1]
// normal matrix, [2] transposition, [3] factorisation, [4] substitutions, [5] store + delta,
// [6] row length, [7] whole
__device__ unsigned *lk_als_phase_buf;
#define LK_PHASE_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define LK_PHASE_ADD(i, a, b) \
    if (lane_id() == 0 && lk_als_phase_buf) lk_als_phase_buf[t * 8 + (i)] = (unsigned)((b) - (a))
#else
#define LK_PHASE_T(var)
#define LK_PHASE_ADD(i, a, b)
#endif

__host__ __device__ constexpr int als_tiles(int NT) { return NT * (NT + 1) / 2; }
// packed index of upper tile (ti <= tj)
__host__ __device__ constexpr int tidx(int ti, int tj) { return tj * (tj + 1) / 2 + ti; }

template <int NT>
struct Gram {
    f32x4 t[als_tiles(NT)];
    float y[NT];
    float yc = 0.f;  // SEQY: the reference's sequential y chain, lane (sub, slot) = feature sub * NT + slot
};

// (inline asm: chained __builtin_amdgcn_permlane*_swap calls are miscompiled by hipcc 7.2 --
// both results of the later swaps land in one register; the s_nop covers the two wait states
// a VALU write of an operand needs before the swap reads it)
__device__ __forceinline__ void swap32(float &a, float &b)
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap16(float &a, float &b)
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// SEQY -- the right-hand side in the REFERENCE's order inside the Gram loop (round 5).  The
// reference forms y as ONE sequential float32 chain per feature, product and sum rounded
// separately (src/accel/als/implicit.rs:116-117; als_rhs.hip); the tuned loop kept four partial
// sums per feature (one per entry slot, fused multiply-adds) and combined them at the end.  On
// the CPU that difference alone explains most of the distance between the two arithmetics on
// rows of a few hundred entries (tools: DESIGN.md section 2): y in the reference's order halves
// it.  A lane holds NT features of ONE entry (its slot); after the 4 x 4 (register x slot)
// transposition -- the two v_permlane32_swap + two v_permlane16_swap of the hybrid solver --
// lane (sub, t) holds the products of the group's FOUR entries for feature sub * NT + t and adds
// them in entry order: bit for bit the reference's chain.  +12 instructions per 4-entry group.
template <int NT>
__device__ __forceinline__ void y_chain_step(float &yc, const float (&q)[NT], const float v1)
{
    float p[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) p[t] = t < NT ? __fmul_rn(q[t < NT ? t : 0], v1) : 0.f;
    swap32(p[0], p[2]);
    swap32(p[1], p[3]);
    swap16(p[0], p[1]);
    swap16(p[2], p[3]);
    yc = __fadd_rn(yc, p[0]);
    yc = __fadd_rn(yc, p[1]);
    yc = __fadd_rn(yc, p[2]);
    yc = __fadd_rn(yc, p[3]);
}

template <int NT>
__device__ __forceinline__ void load_q(const float *p, float (&q)[NT])
{
    if constexpr (NT == 1) {
        q[0] = *p;
    } else if constexpr (NT == 2) {
        f32x2 t = *reinterpret_cast<const f32x2 *>(p);
        q[0] = t.x;
        q[1] = t.y;
    } else {
        static_assert(NT == 4, "Cholesky path supports NT in {1,2,4}");
        f32x4 t = *reinterpret_cast<const f32x4 *>(p);
        q[0] = t.x;
        q[1] = t.y;
        q[2] = t.z;
        q[3] = t.w;
    }
}

// Accumulate CSR entries [beg, end) of one row into G (A tiles and y).
//
// Software pipeline: entries are taken in batches of 64 (one coalesced load of
// indices + values per wave, fetched ONE BATCH AHEAD), each batch is 16 groups of
// 4 entries (= one K=4 MFMA step).  The gathered factor rows live in a RING-slot
// register ring: the gather for group g+RING is issued as soon as group g has been
// consumed -- across batch boundaries too -- so RING x ~320 MFMA cycles of this wave's work,
// plus the other two waves of the SIMD, cover every gather and the wave never drains its
// memory queue inside a row.
template <int NT>
struct GatherRing {
    static constexpr int RING = LK_ALS_RING;  // must divide 16 (groups per batch)
    float q[RING][NT];
    float v[RING];
};

// The batch of 64 (column, value) pairs is staged in wave-private LDS (128 words per batch:
// columns, then values): group g's four entries are then ds_read_b32 at an IMMEDIATE offset
// from one base register.  (A ds_bpermute from the loaded registers needs a distinct address
// register for each of the 16 groups: 16 VGPRs the 4-waves-per-SIMD build does not have.)
template <int NT>
__device__ __forceinline__ void ring_issue(GatherRing<NT> &R, const int slot_idx, const int g,
                                           const float *stage_slot,
                                           const float *__restrict__ other)
{
    constexpr int KP = NT * 16;
    const int lane = lane_id();
    const int col = __builtin_bit_cast(int, stage_slot[g * 4]);
    R.v[slot_idx] = stage_slot[64 + g * 4];
    load_q<NT>(other + (int64_t)col * KP + (lane & 15) * NT, R.q[slot_idx]);
}

template <int NT, bool MASKED, bool SEQY = false, bool WITH_Y = true>
__device__ __forceinline__ void ring_consume(Gram<NT> &G, const GatherRing<NT> &R,
                                             const int slot_idx, const int g, const int nb,
                                             const bool expl)
{
    const int lane = lane_id();
    // MASKED (tail batch only): entries past the row end re-read the row's last entry; kill
    // their q so that neither A (v*q*q) nor y ((v+1)*q) sees them
    const bool live = !MASKED || (g * 4 + (lane >> 4)) < nb;
    const float v = R.v[slot_idx];
    // implicit: A += v q q^T, y += (v + 1) q  (implicit.rs:110-117)
    // explicit: A += q q^T,   y += v q        (explicit.rs:103,109; v = normalised rating)
    const float va = expl ? 1.0f : v;
    float q[NT], a[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        q[t] = live ? R.q[slot_idx][t] : 0.f;
        a[t] = q[t] * va;  // `mtl = mt * vals` (implicit.rs:110-111); exact for va == 1
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int ti = 0; ti <= tj; ++ti)
            G.t[tidx(ti, tj)] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti], q[tj],
                                                                     G.t[tidx(ti, tj)], 0, 0, 0);
    if constexpr (WITH_Y) {
        const float v1 = expl ? v : v + 1.0f;  // `vals += 1.0` (implicit.rs:116)
        if constexpr (SEQY) {
            y_chain_step<NT>(G.yc, q, v1);
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) G.y[t] = fmaf(q[t], v1, G.y[t]);
        }
    }
}

constexpr int GRAM_STAGE_WORDS = 256;  // two batches of 64 (column, value) pairs

template <int NT, bool SEQY = false, bool WITH_Y = true>
__device__ __forceinline__ void gram_accumulate(Gram<NT> &G, const int32_t *__restrict__ cols,
                                                const float *__restrict__ vals, int64_t beg,
                                                int64_t end, const float *__restrict__ other,
                                                int /*ld == 16*NT*/, const bool expl,
                                                float *stage /* GRAM_STAGE_WORDS, wave-private */)
{
    // Every load below is UNCONDITIONAL (out-of-range lanes/groups re-read the row's last
    // entry, which is masked or never consumed): a load inside a branch makes the compiler
    // drain the whole memory queue (s_waitcnt vmcnt(0)) before every MFMA group and the
    // ring would hide nothing.
    const int lane = lane_id();
    constexpr int RING = GatherRing<NT>::RING;
    static_assert(RING >= 1 && RING <= 8 && 16 % RING == 0, "gather ring: 1, 2, 4 or 8 slots");
    GatherRing<NT> R;
    const int64_t last = end - 1;  // end > beg

    // stage_cur / stage_nxt: this lane's view (entry slot = lane >> 4) of the two batch buffers
    float *wr_cur = stage + lane, *wr_nxt = stage + 128 + lane;
    const float *rd_cur = stage + (lane >> 4), *rd_nxt = stage + 128 + (lane >> 4);
    int nxt_col;
    float nxt_val;
    {
        const int64_t e = (beg + lane < end) ? beg + lane : last;
        wr_cur[0] = __builtin_bit_cast(float, cols[e]);
        wr_cur[64] = vals[e];
    }
#pragma unroll
    for (int g = 0; g < RING; ++g) ring_issue<NT>(R, g, g, rd_cur, other);

    int64_t base = beg;
    // full batches: one straight-line body of 16 groups, no branches, no masks
    for (; base + 64 <= end; base += 64) {
        {
            const int64_t e = (base + 64 + lane < end) ? base + 64 + lane : last;
            nxt_col = cols[e];
            nxt_val = vals[e];
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            ring_consume<NT, false, SEQY, WITH_Y>(G, R, g % RING, g, 64, expl);
            if (g == 16 - RING - 2) {
                // the next batch goes to LDS two groups before its first entries are needed
                wr_nxt[0] = __builtin_bit_cast(float, nxt_col);
                wr_nxt[64] = nxt_val;
            }
            if (g < 16 - RING)
                ring_issue<NT>(R, g % RING, g + RING, rd_cur, other);
            else
                ring_issue<NT>(R, g % RING, g + RING - 16, rd_nxt, other);
            // keep the scheduler from hoisting later groups' gathers over this point: the ring
            // depth (and with it the register count) is RING, not whatever fits
            __builtin_amdgcn_sched_barrier(0);
        }
        float *tw = wr_cur;
        wr_cur = wr_nxt;
        wr_nxt = tw;
        const float *tr = rd_cur;
        rd_cur = rd_nxt;
        rd_nxt = tr;
    }
    // tail batch (< 64 entries): wave-uniform branches with no memory operation inside
    if (base < end) {
        const int nb = (int)(end - base);
        const int ngroups = (nb + 3) >> 2;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            if (g < ngroups) ring_consume<NT, true, SEQY, WITH_Y>(G, R, g % RING, g, nb, expl);
            if (g < 16 - RING) ring_issue<NT>(R, g % RING, g + RING, rd_cur, other);
        }
    }
}

// ---- the same accumulation with the gathered rows prefetched into LDS (k = 64 only) ---------
//
// `global_load_lds_dwordx4`: every lane names 16 bytes of a factor row and the memory pipe
// writes them to LDS at M0 + 16 * lane -- one instruction moves a group's four rows (1 KiB)
// without touching a VGPR.  The solver's L image (8.4 KiB) is idle while the normal matrix is
// built, so it holds a ring of DMA_RING = 8 groups = 32 CSR entries in flight per wave, twice
// the register ring, for 20 registers less; the operands come back with one ds_read_b128 per
// lane (each lane reads the 16 bytes "its" load brought: conflict-free by construction).
// hipcc does not count these loads, so the waits are explicit: when group g is consumed the
// groups g+1 .. g+DMA_RING-1 (or fewer at the end of the row) were issued after it, and
// `s_waitcnt vmcnt(that many)` is exactly "group g has landed" (loads retire in order; any
// other memory operation in between only makes the wait more conservative).
#ifndef LK_ALS_DMA_RING
#define LK_ALS_DMA_RING 8
#endif
constexpr int DMA_RING = LK_ALS_DMA_RING;  // (the solve kernel's ring: DMA_RING * 256 floats)

template <int N>
__device__ __forceinline__ void wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// at most `n` (wave-uniform, 0 .. DMA_RING-1) loads still in flight
__device__ __forceinline__ void wait_vm_upto(const int n)
{
    if (n >= 7) wait_vm<7>();
    else if (n == 6) wait_vm<6>();
    else if (n == 5) wait_vm<5>();
    else if (n == 4) wait_vm<4>();
    else if (n == 3) wait_vm<3>();
    else if (n == 2) wait_vm<2>();
    else if (n == 1) wait_vm<1>();
    else wait_vm<0>();
}

// group g of the staged batch -> ring slot `slot_idx` (compile-time)
// WIDE = false: the gathered table is smaller than 4 GiB (decided on the host, per launch), so a
// lane's source is the table's base in an SGPR pair plus ONE 32-bit offset, column * 256 + 16 *
// (lane & 15): a v_lshl_or_b32 where the 64-bit form needs a v_lshlrev_b64 and a v_lshl_add_u64.
// (`other` is a kernel argument: the SGPR pair comes from an s_load, no VALU write precedes its
// use as the base.)
template <bool WIDE>
__device__ __forceinline__ void dma_issue(const unsigned ring_lds, const int slot_idx, const int g,
                                          const float *stage_slot,
                                          const float *__restrict__ other)
{
    const int lane = lane_id();
    const unsigned col = __builtin_bit_cast(unsigned, stage_slot[g * 4]);
    const unsigned dst = ring_lds + slot_idx * 1024;
    unsigned keep;
    if constexpr (WIDE) {
        // one v_mad_u64_u32: (this lane's 16 bytes of row 0) + col * 256
        const uint64_t lane_base = (uint64_t)(uintptr_t)(other + (lane & 15) * 4);
        const float *src = reinterpret_cast<const float *>(lane_base + (uint64_t)col * 256ull);
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(src), "s"(dst)
            : "memory");
    } else {
        const unsigned off = col * 256u + (unsigned)(lane & 15) * 16u;
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(off), "s"(dst), "s"(other)
            : "memory");
    }
}

struct DmaOperand {
    f32x4 q;
    float v;
};
// group g's operands out of the ring (its load must have landed: wait_vm first)
__device__ __forceinline__ DmaOperand dma_fetch(const float *ring, const int slot_idx, const int g,
                                                const float *stage_slot)
{
    DmaOperand o;
    o.q = *reinterpret_cast<const f32x4 *>(ring + slot_idx * 256 + lane_id() * 4);
    o.v = stage_slot[64 + g * 4];
    return o;
}

// SEQY on the DMA path: the reference's y chain WITHOUT the 4 x 4 transposition of y_chain_step.
// The group's four gathered rows still sit in the wave's ring slot when the group is consumed, so
// lane (t, sub) -- which owns the chain of feature sub * 4 + t -- reads that feature's four values
// straight out of them (`rows` = slot + sub * 4 + t, row stride 64 words: the lanes read 64
// consecutive words of a row; two ds_read2st64_b32) and the four multipliers v + 1 (`v1g`: staged
// per batch by gram_accumulate_dma, one broadcast ds_read_b128).  Two packed products and the chain's
// four additions: the same products (each half of a v_pk_mul_f32 is rounded as by v_mul_f32),
// added in the same order, for 6 vector instructions where the transposition took 13.
// MASKED: entries past the row's end are zeros times the multiplier of the row's last entry, as
// in y_chain_step.
template <bool MASKED>
__device__ __forceinline__ void y_chain_lds(float &yc, const float *rows, const float *v1g,
                                            const int g, const int nb)
{
    float q[4] = {rows[0], rows[64], rows[128], rows[192]};
    const f32x4 v1 = *reinterpret_cast<const f32x4 *>(v1g);
    if constexpr (MASKED) {
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = (g * 4 + e) < nb ? q[e] : 0.f;
    }
    f32x2 lo = f32x2{q[0], q[1]} * f32x2{v1.x, v1.y};
    f32x2 hi = f32x2{q[2], q[3]} * f32x2{v1.z, v1.w};
    // (product and sum are rounded separately: nothing may be contracted across this point)
    asm volatile("" : "+v"(lo), "+v"(hi));
    yc = __fadd_rn(yc, lo.x);
    yc = __fadd_rn(yc, lo.y);
    yc = __fadd_rn(yc, hi.x);
    yc = __fadd_rn(yc, hi.y);
}

// the y-chain operands of dma_apply (SEQY): this lane's word of ring slot 0's first row and
// the staged multipliers of the current batch
struct DmaChain {
    const float *rows = nullptr;
    const float *v1 = nullptr;
};

// WITH_Y = false (the chunk kernel of plans whose chunked rows all take y from the reference-order
// chains): no v + 1, no y arithmetic -- the slab's y words are never read
template <bool MASKED, bool SEQY = false, bool WITH_Y = true>
__device__ __forceinline__ void dma_apply(Gram<4> &G, const DmaOperand &o, const int g,
                                          const int nb, const bool expl, const int slot_idx = 0,
                                          const DmaChain ch = DmaChain{})
{
    const int lane = lane_id();
    const bool live = !MASKED || (g * 4 + (lane >> 4)) < nb;
    const float v = o.v;
    const float va = expl ? 1.0f : v;
    float q[4] = {o.q.x, o.q.y, o.q.z, o.q.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) q[t] = live ? q[t] : 0.f;
    // (a[t] stays four scalar products: written as two packed ones with the multiplier
    // broadcast, hipcc packs only where `va` sits in an even register, names its odd neighbour --
    // often the destination of a load in flight -- as the unused half and waits vmcnt(0) for it
    // in front of the MFMAs; with the multiplier in a pair of its own it unpacks most of them
    // again behind the MFMAs and the pair costs a move per group: DESIGN.md section 4.1d)
    float a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = q[t] * va;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int ti = 0; ti <= tj; ++ti)
            G.t[tidx(ti, tj)] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti], q[tj],
                                                                     G.t[tidx(ti, tj)], 0, 0, 0);
    if constexpr (WITH_Y) {
        if constexpr (SEQY) {
            y_chain_lds<MASKED>(G.yc, ch.rows + slot_idx * 256, ch.v1 + g * 4, g, nb);
        } else {
            const float v1 = expl ? v : v + 1.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) G.y[t] = fmaf(q[t], v1, G.y[t]);
        }
    }
}

template <int NT>
__host__ __device__ constexpr int slab_floats();
template <int NT, bool WITH_Y = true>
__device__ __forceinline__ void slab_store(const Gram<NT> &G, float *__restrict__ slab);
template <int NT, bool WITH_Y = true>
__device__ __forceinline__ void gram_zero(Gram<NT> &G);

// ring: RING * 256 floats, stage: GRAM_STAGE_WORDS floats, both wave-private LDS
// `slab` (optional; reference-order work units, als_plan.h): at every 256-entry boundary that is
// followed by more entries the accumulators are stored to *slab (the next slab follows it) and
// start again from zero -- matrixmultiply's KC = 256 blocks, each an fma chain of its own -- while
// the gather ring keeps running: the wave never drains its memory queue inside a unit.  (The
// slab stores count in vmcnt like the loads: the first waits after a boundary are a little more
// conservative than needed, never less.)  The last block of the range is left in G.
// RING: groups in flight (ring: RING * 256 floats); the solve kernel's 8, the chunk kernel's own
// SEQY: `v1s` (2 x 64 floats, wave-private) takes the multipliers v + 1 of the two staged batches
// for y_chain_lds
// WIDE: 64-bit gather addresses (dma_issue)
template <bool SEQY = false, bool WITH_Y = true, int RING = DMA_RING, bool WIDE = true>
__device__ __forceinline__ void gram_accumulate_dma(Gram<4> &G, const int32_t *__restrict__ cols,
                                                    const float *__restrict__ vals, int64_t beg,
                                                    int64_t end, const float *__restrict__ other,
                                                    const bool expl, float *ring, float *stage,
                                                    float *__restrict__ slab = nullptr,
                                                    float *v1s = nullptr)
{
    static_assert(RING == 8 || RING == 4, "DMA ring: 4 or 8 groups");
    const int lane = lane_id();
    const int64_t last = end - 1;  // end > beg
    const unsigned ring_lds =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t) reinterpret_cast<void *>(ring));

    float *wr_cur = stage + lane, *wr_nxt = stage + 128 + lane;
    const float *rd_cur = stage + (lane >> 4), *rd_nxt = stage + 128 + (lane >> 4);
    // (SEQY) the chain's view of the ring -- lane (t, sub): word sub * 4 + t of a row -- and the
    // multiplier buffer of the current batch (wave-uniform; the other one is `yb ^ 64` words on)
    DmaChain ch;
    unsigned yb = 0;
    if constexpr (SEQY && WITH_Y) ch.rows = ring + (lane & 15) * 4 + (lane >> 4);
    {
        const int64_t e = (beg + lane < end) ? beg + lane : last;
        const float v = vals[e];
        wr_cur[0] = __builtin_bit_cast(float, cols[e]);
        wr_cur[64] = v;
        if constexpr (SEQY && WITH_Y) v1s[lane] = expl ? v : v + 1.0f;  // `vals += 1.0`
    }
    // groups of the whole row; group gg lives in batch gg / 16
    const int total = (int)((end - beg + 3) >> 2);
#pragma unroll
    for (int g = 0; g < RING; ++g)
        if (g < total) dma_issue<WIDE>(ring_lds, g, g, rd_cur, other);

    int64_t base = beg;
    int g0 = 0;  // first group of the current batch
    // batches that are followed by at least RING more groups: no guards, constant waits
    for (; g0 + 16 + RING <= total; base += 64, g0 += 16) {
        int nxt_col;
        float nxt_val;
        {
            const int64_t e = (base + 64 + lane < end) ? base + 64 + lane : last;
            nxt_col = cols[e];
            nxt_val = vals[e];
        }
        // operands one group ahead: group g+1 is read out of the ring (its load is the next
        // one to land) before the 10 MFMAs of group g are issued, so the ds_read latency
        // hides behind them.  (Group 0's operands of the NEXT batch are fetched by that
        // batch's first iteration: the pipeline restarts at batch boundaries.)
        wait_vm<RING - 1>();
        DmaOperand cur = dma_fetch(ring, 0, 0, rd_cur);
        if constexpr (SEQY && WITH_Y) ch.v1 = v1s + yb;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            DmaOperand nxt = cur;
            if (g + 1 < 16) {
                wait_vm<RING - 2>();
                nxt = dma_fetch(ring, (g + 1) % RING, g + 1, rd_cur);
            }
            dma_apply<false, SEQY, WITH_Y>(G, cur, g, 64, expl, g % RING, ch);
            if (g == 16 - RING - 2) {
                wr_nxt[0] = __builtin_bit_cast(float, nxt_col);
                wr_nxt[64] = nxt_val;
                if constexpr (SEQY && WITH_Y) {
                    // (the value is waited for HERE, with the writes above: hoisted, the addition
                    // would drain the memory queue groups earlier)
                    asm volatile("" : "+v"(nxt_val));
                    v1s[(yb ^ 64) + lane] = expl ? nxt_val : nxt_val + 1.0f;
                }
            }
            if (g < 16 - RING)
                dma_issue<WIDE>(ring_lds, g % RING, g + RING, rd_cur, other);
            else
                dma_issue<WIDE>(ring_lds, g % RING, g + RING - 16, rd_nxt, other);
            cur = nxt;
            __builtin_amdgcn_sched_barrier(0);
        }
        if (slab && ((g0 + 16) & 63) == 0) {  // (wave-uniform) a 256-entry block is complete
            slab_store<4, WITH_Y>(G, slab);
            slab += slab_floats<4>();
            gram_zero<4, WITH_Y>(G);
        }
        float *tw = wr_cur;
        wr_cur = wr_nxt;
        wr_nxt = tw;
        const float *tr = rd_cur;
        rd_cur = rd_nxt;
        rd_nxt = tr;
        yb ^= 64;
    }
    // the last batches: the same body -- no masks, operands one group ahead -- under wave-uniform
    // guards (scalar compares and branches only), with waits that shrink towards the end of the
    // row.  Only the row's LAST group can hold entries past the row's end: it alone is consumed
    // masked, where its batch ends, its ring slot and staged words found by a run-time index.
    for (; g0 < total; base += 64, g0 += 16) {
        const int nb = (int)((end - base < 64) ? end - base : 64);
        const int rem = total - 1 - g0;     // groups of this batch in front of the row's last one
        const bool more = g0 + 16 < total;  // another batch follows (then rem >= 16)
        int nxt_col = 0;
        float nxt_val = 0.f;
        if (more) {
            const int64_t e = (base + 64 + lane < end) ? base + 64 + lane : last;
            nxt_col = cols[e];
            nxt_val = vals[e];
        }
        if constexpr (SEQY && WITH_Y) ch.v1 = v1s + yb;
        DmaOperand cur{};
        if (rem > 0) {
            // group g0 has landed when only the groups issued after it are in flight
            wait_vm_upto(rem < RING - 1 ? rem : RING - 1);
            cur = dma_fetch(ring, 0, 0, rd_cur);
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            if (g < rem) {
                DmaOperand nxt = cur;
                if (g + 1 < 16) {
                    // (only the wait is guarded: where group g + 1 is the row's last one, which
                    // is fetched again below, its slot is read for nothing -- one ds_read per
                    // row against the five moves per group of a conditional `nxt`)
                    if (g + 1 < rem) {
                        const int later = rem - 1 - g;  // groups issued after group g + 1
                        wait_vm_upto(later < RING - 2 ? later : RING - 2);
                    }
                    nxt = dma_fetch(ring, (g + 1) % RING, g + 1, rd_cur);
                }
                dma_apply<false, SEQY, WITH_Y>(G, cur, g, 64, expl, g % RING, ch);
                if (g == 16 - RING - 2 && more) {
                    wr_nxt[0] = __builtin_bit_cast(float, nxt_col);
                    wr_nxt[64] = nxt_val;
                    if constexpr (SEQY && WITH_Y) {
                        // (the value is waited for HERE, with the writes above: hoisted, the
                        // addition would drain the memory queue groups earlier)
                        asm volatile("" : "+v"(nxt_val));
                        v1s[(yb ^ 64) + lane] = expl ? nxt_val : nxt_val + 1.0f;
                    }
                }
                if (g + RING <= rem) {  // group g0 + g + RING exists
                    if (g < 16 - RING)
                        dma_issue<WIDE>(ring_lds, g % RING, g + RING, rd_cur, other);
                    else
                        dma_issue<WIDE>(ring_lds, g % RING, g + RING - 16, rd_nxt, other);
                }
                cur = nxt;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (rem < 16) {  // the row ends in this batch: nothing is in flight behind its last group
            const int slot_idx = rem & (RING - 1);
            wait_vm<0>();
            dma_apply<true, SEQY, WITH_Y>(G, dma_fetch(ring, slot_idx, rem, rd_cur), rem, nb, expl,
                                          slot_idx, ch);
        }
        if (slab && ((g0 + 16) & 63) == 0 && g0 + 16 < total) {  // a block boundary, more follows
            slab_store<4, WITH_Y>(G, slab);
            slab += slab_floats<4>();
            gram_zero<4, WITH_Y>(G);
        }
        float *tw = wr_cur;
        wr_cur = wr_nxt;
        wr_nxt = tw;
        const float *tr = rd_cur;
        rd_cur = rd_nxt;
        rd_nxt = tr;
        yb ^= 64;
    }
}

// ---- a FULL 256-entry chunk (k = 64) ---------------------------------------------------------
// Reference-order rows are cut into matrixmultiply's KC = 256 blocks (als_plan.h): every chunk of
// such a row but its last has exactly 256 entries = 64 groups = 4 batches.  The general routine
// above sends the last batch of any range down its guarded path (wave-uniform tests, waits that
// shrink, the last group masked); for a 256-entry chunk that is a quarter of the work.  Here the
// batch loop is unrolled
// over the four batches, so every guard and every wait count is a compile-time constant.  Same
// operations in the same order: bit-identical to gram_accumulate_dma on the same range.
template <bool WITH_Y = true, int RING = DMA_RING, bool WIDE = true>
__device__ __forceinline__ void gram_accumulate_dma_256(Gram<4> &G, const int32_t *__restrict__ cols,
                                                        const float *__restrict__ vals, int64_t beg,
                                                        const float *__restrict__ other,
                                                        const bool expl, float *ring, float *stage)
{
    constexpr int TOTAL = 64;
    const int lane = lane_id();
    const unsigned ring_lds =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t) reinterpret_cast<void *>(ring));
    float *const wr0 = stage + lane, *const wr1 = stage + 128 + lane;
    const float *const rd0 = stage + (lane >> 4), *const rd1 = stage + 128 + (lane >> 4);
    wr0[0] = __builtin_bit_cast(float, cols[beg + lane]);
    wr0[64] = vals[beg + lane];
#pragma unroll
    for (int g = 0; g < RING; ++g) dma_issue<WIDE>(ring_lds, g, g, rd0, other);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float *const wr_nxt = (b & 1) ? wr0 : wr1;
        const float *const rd_cur = (b & 1) ? rd1 : rd0, *const rd_nxt = (b & 1) ? rd0 : rd1;
        int nxt_col = 0;
        float nxt_val = 0.f;
        if (b < 3) {
            nxt_col = cols[beg + 64 * (b + 1) + lane];
            nxt_val = vals[beg + 64 * (b + 1) + lane];
        }
        {
            const int later = TOTAL - 1 - 16 * b;
            wait_vm_upto(later < RING - 1 ? later : RING - 1);
        }
        DmaOperand cur = dma_fetch(ring, 0, 0, rd_cur);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int gg = 16 * b + g;
            DmaOperand nxt = cur;
            if (g + 1 < 16) {
                // group gg + 1 must have landed: the groups issued after it are still in flight
                const int later = TOTAL - 1 - (gg + 1);
                const int issued_after = (gg + RING < TOTAL ? gg + RING - 1 : TOTAL - 1) - (gg + 1);
                wait_vm_upto(issued_after < later ? issued_after : later);
                nxt = dma_fetch(ring, (g + 1) % RING, g + 1, rd_cur);
            }
            dma_apply<false, false, WITH_Y>(G, cur, g, 64, expl);
            if (g == 16 - RING - 2 && b < 3) {
                wr_nxt[0] = __builtin_bit_cast(float, nxt_col);
                wr_nxt[64] = nxt_val;
            }
            if (gg + RING < TOTAL) {
                if (g < 16 - RING)
                    dma_issue<WIDE>(ring_lds, g % RING, g + RING, rd_cur, other);
                else
                    dma_issue<WIDE>(ring_lds, g % RING, g + RING - 16, rd_nxt, other);
            }
            cur = nxt;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// slab layout: tile e as [64 lanes][4 registers] (one 16-byte store / load per lane and tile:
// a slab is written in als_tiles + 1 instructions where the register-major layout took 4 x as
// many -- it matters since round 5, when a wave stores a slab every 256 entries), then y as
// [64 lanes][NT]
template <int NT>
__host__ __device__ constexpr int slab_floats()
{
    return (als_tiles(NT) * 4 + NT) * 64;
}

template <int NT, bool WITH_Y>
__device__ __forceinline__ void slab_store(const Gram<NT> &G, float *__restrict__ slab)
{
    const int lane = lane_id();
    // (streaming stores -- a slab is written once and read once by another kernel; kept out of
    // the L2 it would otherwise share with the gathered factor rows)
#pragma unroll
    for (int e = 0; e < als_tiles(NT); ++e)
        __builtin_nontemporal_store(G.t[e], reinterpret_cast<f32x4 *>(slab + (e * 64 + lane) * 4));
    if constexpr (WITH_Y) {
#pragma unroll
        for (int t = 0; t < NT; ++t) slab[als_tiles(NT) * 256 + lane * NT + t] = G.y[t];
    }
}

// WITH_Y = false: the tiles only (the y words of such a slab may never have been written)
template <int NT, bool WITH_Y = true>
__device__ __forceinline__ void slab_add(Gram<NT> &G, const float *__restrict__ slab)
{
    const int lane = lane_id();
#pragma unroll
    for (int e = 0; e < als_tiles(NT); ++e)
        G.t[e] += *reinterpret_cast<const f32x4 *>(slab + (e * 64 + lane) * 4);
    if constexpr (WITH_Y) {
#pragma unroll
        for (int t = 0; t < NT; ++t) G.y[t] += slab[als_tiles(NT) * 256 + lane * NT + t];
    }
}

template <int NT, bool WITH_Y>
__device__ __forceinline__ void gram_zero(Gram<NT> &G)
{
#pragma unroll
    for (int e = 0; e < als_tiles(NT); ++e) G.t[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (WITH_Y) {
#pragma unroll
        for (int t = 0; t < NT; ++t) G.y[t] = 0.f;
    }
}

// ---- slab groups: slab[head] += slab[head + 1] + ... + slab[head + cnt - 1] ------------------
// (grid: groups x ceil(sum_floats / 1024); float4 per thread; chunk order inside the group;
// only the first sum_floats words of a slab are summed -- all of it, or the tiles without y)
__global__ __launch_bounds__(256) void slab_group_reduce_kernel(float *__restrict__ slabs,
                                                                int64_t slab_floats,
                                                                int64_t sum_floats,
                                                                const int32_t *__restrict__ grp_head,
                                                                const int32_t *__restrict__ grp_cnt,
                                                                int parts)
{
    const int g = blockIdx.x / parts;
    const int64_t e = ((int64_t)(blockIdx.x - g * parts) * 256 + threadIdx.x) * 4;
    if (e >= sum_floats) return;
    float *head = slabs + (size_t)grp_head[g] * slab_floats + e;
    const int cnt = grp_cnt[g];
    f32x4 acc = *reinterpret_cast<const f32x4 *>(head);
    int c = 1;
    // (reference-order rows are ONE group of up to thousands of slabs: eight loads in flight,
    // the additions strictly in chunk order)
    for (; c + 8 <= cnt; c += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = __builtin_nontemporal_load(
                reinterpret_cast<const f32x4 *>(head + (size_t)(c + u) * slab_floats));
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; c < cnt; ++c)
        acc += *reinterpret_cast<const f32x4 *>(head + (size_t)c * slab_floats);
    *reinterpret_cast<f32x4 *>(head) = acc;
}

int launch_slab_group_reduce(const lk_als_plan *p, float *slabs, size_t slab_floats, hipStream_t st,
                             size_t sum_floats)
{
    if (p->n_groups <= 0) return LK_OK;
    if (sum_floats == 0) sum_floats = slab_floats;
    const int parts = (int)((sum_floats / 4 + 255) / 256);
    hipLaunchKernelGGL(slab_group_reduce_kernel, dim3((unsigned)(p->n_groups * parts)), dim3(256),
                       0, st, slabs, (int64_t)slab_floats, (int64_t)sum_floats, p->d_grp_head,
                       p->d_grp_cnt, parts);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// ---- chunk kernel: one wave per chunk of a long row ------------------------
// The chunk kernel's own DMA ring depth (4 or 8 groups): its LDS -- 4 waves x (stage + ring) --
// decides how many of its workgroups a CU holds.  8 deep: 36 864 B, four per CU; 4 deep: 20 480 B,
// the five per CU that the registers of the kernel without y allow (36 + 60 accumulation
// registers).  The 4-deep ring was measured and bought nothing: 8 it is.
#ifndef LK_ALS_CHUNK_RING
#define LK_ALS_CHUNK_RING 8
#endif
constexpr int CHUNK_RING = LK_ALS_CHUNK_RING;

template <int NT>
__host__ __device__ constexpr int chunk_lds_floats()
{
    return GRAM_STAGE_WORDS + (NT == 4 ? CHUNK_RING * 256 : 0);
}

// chunk workgroups a CU holds at padded k = 64: LDS (160 KiB per CU), at most the 5 waves per
// SIMD its registers allow (als_plan.hip sizes the work units of hybrid plans by it)
int als_chol_chunk_wgs_per_cu()
{
    const int by_lds = (int)(160 * 1024 / (4 * chunk_lds_floats<4>() * sizeof(float)));
    return by_lds < 5 ? by_lds : 5;
}

// WITH_Y = false: the slabs carry the tiles only (chol_front)
// WIDE (padded k = 64 only): 64-bit gather addresses, for tables of 4 GiB and more (dma_issue)
template <int NT, bool EXPL, bool WITH_Y, bool WIDE>
__device__ __forceinline__ void als_chunk_body(
    const int32_t *__restrict__ indices, const float *__restrict__ values,
    const int64_t *__restrict__ chunk_beg, const int32_t *__restrict__ chunk_len,
    int64_t n_chunks, const float *__restrict__ other, int ld, float *__restrict__ slabs,
    const int64_t blk, float *__restrict__ lds_flat,
    const int32_t *__restrict__ chunk_slab = nullptr, const int block_len = 0)
{
    constexpr bool DMA = NT == 4;
    float(*stage_all)[chunk_lds_floats<NT>()] =
        reinterpret_cast<float(*)[chunk_lds_floats<NT>()]>(lds_flat);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = blk * 4 + wave;
    if (c >= n_chunks) return;
    Gram<NT> G;
    gram_zero<NT, WITH_Y>(G);
    const int64_t beg = chunk_beg[c];
    // the unit's first slab (a unit of several 256-entry blocks stores one slab per block)
    float *slab = slabs + (size_t)(chunk_slab ? chunk_slab[c] : c) * slab_floats<NT>();
    if constexpr (DMA) {
        const int len = chunk_len[c];
        if (block_len == 256 && len > 256) {  // (wave-uniform) a reference-order work unit
            gram_accumulate_dma<false, WITH_Y, CHUNK_RING, WIDE>(
                G, indices, values, beg, beg + len, other, EXPL,
                stage_all[wave] + GRAM_STAGE_WORDS, stage_all[wave], slab);
            slab += (size_t)((len - 1) >> 8) * slab_floats<NT>();  // the last block is still in G
        } else if (len == 256)  // a full reference-order block
            gram_accumulate_dma_256<WITH_Y, CHUNK_RING, WIDE>(
                G, indices, values, beg, other, EXPL, stage_all[wave] + GRAM_STAGE_WORDS,
                stage_all[wave]);
        else
            gram_accumulate_dma<false, WITH_Y, CHUNK_RING, WIDE>(
                G, indices, values, beg, beg + len, other, EXPL,
                stage_all[wave] + GRAM_STAGE_WORDS, stage_all[wave]);
    } else
        gram_accumulate<NT, false, WITH_Y>(G, indices, values, beg, beg + chunk_len[c], other, ld,
                                           EXPL, stage_all[wave]);
    slab_store<NT, WITH_Y>(G, slab);
}

template <int NT, bool EXPL, bool WITH_Y, bool WIDE = false>
__global__ __launch_bounds__(256) void als_chunk_kernel(
    const int32_t *__restrict__ indices, const float *__restrict__ values,
    const int64_t *__restrict__ chunk_beg, const int32_t *__restrict__ chunk_len,
    int64_t n_chunks, const float *__restrict__ other, int ld, float *__restrict__ slabs,
    const int32_t *__restrict__ chunk_slab, int block_len)
{
    __shared__ __attribute__((aligned(16))) float lds_flat[4 * chunk_lds_floats<NT>()];
    als_chunk_body<NT, EXPL, WITH_Y, WIDE>(indices, values, chunk_beg, chunk_len, n_chunks, other, ld,
                                     slabs, (int64_t)blockIdx.x, lds_flat, chunk_slab, block_len);
}

// ---- solve: the packed L image ---------------------------------------------------------------
//
// The solver's LDS: KP reciprocal pivots | extraction scratch (64 lanes x 4) | L image.
// Packed strictly-lower image: column j holds rows c in [c0(j), KP), c0 = (j+1)&~3 (16-byte
// aligned segments), the columns at DESCENDING addresses: column 0 ends the image, column j + 1
// lies directly below column j.  off(j) is the word of row c0(j) of column j.
// Why descending: at KP = 64 every lane stores its lj of column j at off(j) - c0(j) + lane -- one
// address register plus an immediate, no per-column address select.  The lanes below the stored
// segment (rows < c0(j)) land on the words right below it: the segments of the columns j + 1 ..,
// which are stored later, or -- for the last columns -- up to 60 words of the extraction scratch
// in front of the image, which is dead between a panel's extraction and the next one.
template <int KP>
struct LPack {
    __host__ __device__ static constexpr int c0(int j) { return (j + 1) & ~3; }
    // words of the columns 0 .. j-1: 4*KP*m - 8m^2 + 4m + r*(KP - 4m), j = 4m + r
    __host__ __device__ static constexpr int before(int j)
    {
        const int m = j >> 2, r = j & 3;
        return 4 * KP * m - 8 * m * m + 4 * m + r * (KP - 4 * m);
    }
    static constexpr int SIZE = KP * KP / 2 + KP;  // words of the image
    static constexpr int RINV = 0, SCR = KP, IMG = KP + 256;
    __host__ __device__ static constexpr int off(int j)
    {
        return IMG + SIZE - before(j) - (KP - c0(j));
    }
};
static_assert(LPack<64>::off(62) - LPack<64>::c0(62) >= LPack<64>::SCR &&
                  LPack<64>::off(0) + 64 == LPack<64>::IMG + LPack<64>::SIZE &&
                  LPack<64>::off(63) == LPack<64>::IMG,
              "L image: the stores of all 64 lanes stay between the scratch and the image's end");

// ---- hybrid Cholesky ---------------------------------------------------------------------------
//
// The matrix stays in the accumulator tiles; panels of FOUR columns J .. J+3 are
//   E. extracted into the lane = row layout (lane i: A'[i][J .. J+3]; by symmetry these are the
//      four registers of row group MG of the tiles (TJ, t): one masked ds_write_b128 per tile,
//      one ds_read_b128 per lane),
//   F. factored there with registers and v_readlane only (no LDS in the dependent chain); the
//      forward substitution rides along and every finished column goes to the strictly-lower
//      L image of the back substitution,
//   C. turned into MFMA operands by a 4 x 4 (register x row group) transposition made of two
//      v_permlane32_swap and two v_permlane16_swap: q[t], lane (s, c) = L[16 t + c][J + s],
//   U. applied to everything right of the panel: ONE v_mfma_f32_16x16x4_f32 per tile with
//      -q[ti] as the A operand and q[tj] as the B operand.
// tools/emul/hybrid_chol.py is the lane-level NumPy model of this; tools/ub/permlane_swap.hip
// checks the swap semantics on the device.
template <int NT>
__host__ __device__ constexpr int hybrid_lds_floats()
{
    // KP reciprocal pivots | extraction scratch (64 lanes x 4) | L image (LPack)
    return LPack<NT * 16>::SIZE + NT * 16 + 256;
}

// The lane sets of the solver are compile-time constants: 64-bit masks that the scalar unit moves
// into an SGPR pair (`__builtin_amdgcn_inverse_ballot_w64`), where `lane > j` cost a v_cmp each.
// lanes_above(j): the lanes j + 1 .. 63; lanes_below(j): the lanes 0 .. j - 1.
__host__ __device__ constexpr unsigned long long lanes_above(int j)
{
    return j >= 63 ? 0ull : ~0ull << (j + 1);
}
__host__ __device__ constexpr unsigned long long lanes_below(int j)
{
    return j >= 64 ? ~0ull : (1ull << j) - 1;
}
static_assert(lanes_above(-1) == ~0ull && lanes_above(0) == ~1ull && lanes_above(62) == 1ull << 63 &&
                  lanes_above(63) == 0 && lanes_below(0) == 0 && lanes_below(63) == ~0ull >> 1 &&
                  lanes_below(64) == ~0ull,
              "lane masks: lane > j and lane < j for every j the solver asks");

template <int NT, int M>
__device__ __forceinline__ void hybrid_step(Gram<NT> &G, float &b, float &minpiv,
                                            float *__restrict__ lds, const int lane, const int ew,
                                            const int rz)
{
    constexpr int KP = NT * 16, J = 4 * M, TJ = M >> 2, MG = M & 3;
    using P = LPack<KP>;
    const int slot = lane >> 4;
    float *rinvarr = lds + P::RINV;
    float *scr = lds + P::SCR;

    // E. extraction
#pragma unroll
    for (int t = TJ; t < NT; ++t)
        if (slot == MG)  // (ew = 4 (lane & 15), held in a register: the tile is an immediate)
            *reinterpret_cast<f32x4 *>(&scr[t * 64 + ew]) = G.t[tidx(TJ, t)];
    // (the zeroed quad and the masked read stay: with every lane reading -- the lanes left of the
    // panel would get stale words that the column masks discard below -- the half-epoch once no
    // longer reproduced its recorded bits, for a reason not found: DESIGN.md sections 4.1d, 4.1f)
    f32x4 pv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (__builtin_amdgcn_inverse_ballot_w64(lanes_above(16 * TJ - 1) & lanes_below(KP)))
        pv = *reinterpret_cast<const f32x4 *>(&scr[lane * 4]);
    float pr[4] = {pv.x, pv.y, pv.z, pv.w};

    // F. the four columns
    float lp[4];
#pragma unroll
    for (int s0 = 0; s0 < 4; ++s0) {
        const int j = J + s0;
        const float piv = bcast(pr[s0], j);
        minpiv = fminf(minpiv, piv);
        const float rinv = __builtin_amdgcn_rsqf(piv);
        // (no exec-mask round trips in the column loop: rinv is wave-uniform, every lane stores
        // the same value to the same word; at KP = 64 every lane stores its lj at the column's
        // base + lane -- LPack says where the lanes outside the stored segment land; narrower
        // systems leave lanes past KP, which aim at their own word of the extraction scratch,
        // dead until the next panel; rz = 0 in a register spares a v_mov_b32 of the base per panel)
        rinvarr[j + rz] = rinv;
        // strictly-lower column j: exactly +0 in the lanes at and above the diagonal
        const float lj = __builtin_amdgcn_inverse_ballot_w64(lanes_above(j)) ? pr[s0] * rinv : 0.f;
        if (j + 1 < KP) {
            if constexpr (KP == 64) {
                lds[P::off(j) - P::c0(j) + lane] = lj;
            } else {
                const bool in = lane >= P::c0(j) && lane < KP;
                float *dst = in ? &lds[P::off(j) + lane - P::c0(j)] : &scr[lane];
                *dst = lj;
            }
        }
        // forward substitution: z_j = y_j / L_jj, y -= L[:, j] z_j
        const float zj = bcast(b, j) * rinv;
        b = fmaf(-lj, zj, b);
#pragma unroll
        for (int s = s0 + 1; s < 4; ++s) pr[s] = fmaf(-lj, bcast(lj, J + s), pr[s]);
        lp[s0] = lj;
    }
    if constexpr (J + 4 < KP) {
        // C. register x row-group transposition: lp[s] @ group t  ->  q[t] @ group s
        swap32(lp[0], lp[2]);
        swap32(lp[1], lp[3]);
        swap16(lp[0], lp[1]);
        swap16(lp[2], lp[3]);
        // U. rank-4 update (tile row TJ first: the next panel is extracted from it)
        float nq[NT];
#pragma unroll
        for (int t = TJ; t < NT; ++t) nq[t] = -lp[t];
#pragma unroll
        for (int ti = TJ; ti < NT; ++ti)
#pragma unroll
            for (int t2 = ti; t2 < NT; ++t2)
                G.t[tidx(ti, t2)] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    nq[ti], lp[t2], G.t[tidx(ti, t2)], 0, 0, 0);
    }
}

template <int NT, int... Ms>
__device__ __forceinline__ void hybrid_steps(Gram<NT> &G, float &b, float &minpiv,
                                             float *__restrict__ lds, const int lane,
                                             const int ew, const int rz,
                                             std::integer_sequence<int, Ms...>)
{
    (hybrid_step<NT, Ms>(G, b, minpiv, lds, lane, ew, rz), ...);
}

// G: accumulator tiles of A' and the right-hand side (every lane: y'[16 t + sub]).  Returns
// the smallest pivot; b = solution for primed row `lane`.
template <int NT>
__device__ __forceinline__ float hybrid_solve(Gram<NT> &G, float &b, float *__restrict__ lds
#ifdef LK_ALS_PHASES
                                              ,
                                              unsigned long long *tmid
#endif
)
{
    constexpr int KP = NT * 16;
    using P = LPack<KP>;
    // the lane number is made opaque here so that nothing derived from it for the solver
    // (row-group masks, LDS addresses) is kept alive across the normal-matrix loop
    int lane = lane_id();
    asm volatile("" : "+v"(lane));
    // rhs for primed row `lane`: tile lane >> 4, sub lane & 15 -> G.y[lane >> 4] of this lane
    b = 0.f;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) b = ((lane >> 4) == tt) ? G.y[tt] : b;
    float minpiv = 3.0e38f;
    // word of this lane's quad in a tile's part of the extraction scratch, and a zero: opaque, so
    // that the addresses made of them are formed once and not again in every panel
    int ew = (lane & 15) * 4, rz = 0;
    asm volatile("" : "+v"(ew), "+v"(rz));
    hybrid_steps<NT>(G, b, minpiv, lds, lane, ew, rz, std::make_integer_sequence<int, KP / 4>{});
#ifdef LK_ALS_PHASES
    asm volatile("" : "+v"(b));
    *tmid = __builtin_amdgcn_s_memtime();
#endif
    // backward: L^T x = z, lane = primed row (z = b / L_jj after the folded forward pass)
    const float dinv = (lane < KP) ? lds[P::RINV + lane] : 0.f;
    b *= dinv;
    const int my_c0 = (lane + 1) & ~3;
    const float *mycol = lds + P::off(lane) - my_c0;
#pragma unroll
    for (int j4 = KP / 4 - 1; j4 >= 0; --j4) {
        // (lane < KP - 1 && 4 * j4 >= my_c0: the lanes 0 .. min(4 j4 + 2, KP - 2))
        const int top = 4 * j4 + 3 < KP - 1 ? 4 * j4 + 3 : KP - 1;
        f32x4 l4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (__builtin_amdgcn_inverse_ballot_w64(lanes_below(top)))
            l4 = *reinterpret_cast<const f32x4 *>(mycol + 4 * j4);
#pragma unroll
        for (int u = 3; u >= 0; --u) {
            const int j = 4 * j4 + u;
            if (j >= 1) {
                const float xj = bcast(b * dinv, j);
                b = fmaf(-l4[u], xj, b);
            }
        }
    }
    b *= dinv;
    return minpiv;
}

// EXPL: explicit-feedback model (explicit.rs) instead of the implicit one (implicit.rs); a
// template parameter so that the implicit instantiation carries nothing of it
// CTL: poll the task-control block (cancel) before the row and count it when done; a
// template parameter so that the uncontrolled instantiation -- the training engine's -- is
// instruction for instruction the tuned kernel
// YREF: take the right-hand side from `y_ref` ([tasks x KP], indexed by the TASK t of this launch's
// order, natural feature order; als_rhs.hip:
// the reference's summation order) instead of the accumulated one; a template parameter so that
// the default instantiation is instruction for instruction the tuned kernel
// SEQY: rows that form their own right-hand side do it in the reference's order (y_chain_step); a
// template parameter so that LK_ALS_RHS_ORDER=accurate keeps round 4's kernel instruction for
// instruction
// WIDE (padded k = 64 only): 64-bit gather addresses, for tables of 4 GiB and more (dma_issue)
template <int NT, bool IS64, bool EXPL, bool CTL, bool YREF, bool SEQY, bool WIDE>
__device__ __forceinline__ void als_solve_body(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ indices,
    const float *__restrict__ values, const int32_t *__restrict__ order, int64_t n_rows,
    const int32_t *__restrict__ row_slab, const float *__restrict__ other, int ld_other,
    float *__restrict__ this_, int ld_this, const float *__restrict__ otor_p,
    const float *__restrict__ slabs, float *__restrict__ row_delta, int *__restrict__ status,
    int k, float reg, TaskCtlDev ctl, const float *__restrict__ y_ref, int chunk_rt,
    const int64_t blk, float *__restrict__ lds_flat)
{
    constexpr int KP = NT * 16;
    float(*lds_all)[hybrid_lds_floats<NT>()] =
        reinterpret_cast<float(*)[hybrid_lds_floats<NT>()]>(lds_flat);

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int sub = lane & 15, slot = lane >> 4;
    const int64_t t = blk * 4 + wave;
    if (t >= n_rows) return;
    LK_PHASE_T(ph0);
    if constexpr (CTL) {
        // AccelTask.cancel (src/accel/tasks/mod.rs:88-95): rows not started yet are skipped
        int c = 0;
        if (lane == 0) c = ctl_cancelled(ctl, (blk & 63) == 0 && wave == 0) ? 1 : 0;
        if (__builtin_amdgcn_readfirstlane(c)) return;
    }
    const int row = order[t];
    const int64_t beg = indptr[row], end = indptr[row + 1];
    float *lds = lds_all[wave];

    // feature owned by this lane in the lane==row phase
    const int my_f = (lane & 15) * NT + (lane >> 4);
    const bool my_valid = (lane < KP) && (my_f < k);
    float *xrow = this_ + (int64_t)row * ld_this;

    if (end == beg) {  // implicit.rs:98-101
        if (lane < KP) xrow[lane] = 0.f;
        if (lane == 0) row_delta[row] = 0.f;
        if constexpr (CTL)
            if (lane == 0) ctl_advance(ctl, 1);
        return;
    }

    LK_PHASE_T(ph1);
    Gram<NT> G;
    // start from OtOr (primed, padded with identity on the pad features)
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int ti = 0; ti <= tj; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                G.t[tidx(ti, tj)][r] = otor_p[(ti * 16 + slot * 4 + r) * KP + tj * 16 + sub];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) G.y[tt] = 0.f;

    const int first_slab = row_slab[row];
    if (first_slab >= 0) {
        const int64_t n = end - beg;
        // (reference-order plans, YREF only: 256-entry chunks whose slabs were summed one after
        // the other into the row's first slab -- that one is added, after OtOr: a = otor + mtm)
        const bool refo = YREF && chunk_rt > 0;
        const int ch = refo ? chunk_rt : LK_ALS_CHUNK;
        const int ns = (int)((n + ch - 1) / ch);
        // many chunks: the groups were pre-summed into their heads (slab_group_reduce_kernel)
        const int step = refo ? ns : (ns > LK_ALS_SLAB_GROUP ? LK_ALS_SLAB_GROUP : 1);
        for (int s = 0; s < ns; s += step)
            // (YREF: y comes from y_ref below; the slab's y words may never have been written)
            slab_add<NT, !YREF>(G, slabs + (size_t)(first_slab + s) * slab_floats<NT>());
    } else {
        // (the solver's LDS is idle while the normal matrix is built: it stages the CSR
        // batches and, for k = 64, holds the ring of prefetched factor rows)
        // (ring: words 0 .. 2047, staged batches: the last 256; the 128 words between them are
        // idle as well and take the y chain's multipliers)
        if constexpr (NT == 4) {
            static_assert(NT != 4 || DMA_RING * 256 + 128 <= LPack<KP>::SIZE + KP, "v + 1 staging");
            gram_accumulate_dma<SEQY && !YREF, true, DMA_RING, WIDE>(
                G, indices, values, beg, end, other, EXPL, lds, lds + LPack<KP>::SIZE + KP,
                nullptr, lds + DMA_RING * 256);
        }
        else
            gram_accumulate<NT, SEQY && !YREF>(G, indices, values, beg, end, other, ld_other,
                                               EXPL, lds);
    }
    if (EXPL) {
        // explicit.rs:104-107: mtm[i][i] += reg * n, AFTER the product, real features only
        // (the pad features keep the identity they got from otor_p)
        const float dg = reg * (float)(end - beg);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (slot * 4 + r == sub && (slot * 4 + r) * NT + ti < k) G.t[tidx(ti, ti)][r] += dg;
    }

#ifdef LK_ALS_PHASES
    asm volatile("" : "+v"(G.t[0]), "+v"(G.t[als_tiles(NT) - 1]));
#endif
    LK_PHASE_T(ph2);
    if (SEQY && !YREF && first_slab < 0) {
        // the chain of feature sub * NT + tt lives in lane (sub, slot = tt): hand it to every slot
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) G.y[tt] = __shfl(G.yc, sub + 16 * tt, 64);
    } else {
        // y: combine the 4 entry slots -> every lane has the full y for feature (t, sub)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            G.y[tt] += __shfl_xor(G.y[tt], 16, 64);
            G.y[tt] += __shfl_xor(G.y[tt], 32, 64);
        }
    }
    if constexpr (YREF) {
        // primed (tt, sub) <-> feature sub * NT + tt; pad features carry y = 0 (their factor
        // columns are zero, so the reference-order sum over them is exactly 0 as well)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) G.y[tt] = y_ref[(int64_t)t * KP + sub * NT + tt];
    }
    const float old = my_valid ? xrow[my_f] : 0.f;
    float b;
#ifdef LK_ALS_PHASES
    LK_PHASE_T(ph3);
    unsigned long long ph4 = 0;
    const float minpiv = hybrid_solve<NT>(G, b, lds, &ph4);
    asm volatile("" : "+v"(b));
    LK_PHASE_T(ph5);
#else
    const float minpiv = hybrid_solve<NT>(G, b, lds);
#endif
    // not SPD: a non-positive pivot, or NaN/Inf anywhere in the solution
    const bool bad = !(minpiv > 0.f) || (my_valid && !(fabsf(b) <= 3.0e38f));
    if (__any(bad) && lane == 0) atomicCAS(status, 0, row + 1);

    float d = 0.f;
    if (my_valid) {
        xrow[my_f] = b;
        d = b - old;
    }
    const float d2 = wave_sum(d * d);
    if (lane == 0) row_delta[row] = d2;
    if constexpr (CTL)
        if (lane == 0) ctl_advance(ctl, 1);  // progress unit = rows (tasks/mod.rs:97-105)
#ifdef LK_ALS_PHASES
    LK_PHASE_T(ph6);
    LK_PHASE_ADD(0, ph0, ph1);
    LK_PHASE_ADD(1, ph1, ph2);
    LK_PHASE_ADD(2, ph2, ph3);
    LK_PHASE_ADD(3, ph3, ph4);
    LK_PHASE_ADD(4, ph4, ph5);
    LK_PHASE_ADD(5, ph5, ph6);
    LK_PHASE_ADD(6, (unsigned long long)beg, (unsigned long long)end);
    LK_PHASE_ADD(7, ph0, ph6);
#endif
}

// the hybrid solver keeps the matrix in its 40 accumulator registers: 4 waves per SIMD
template <int NT, bool IS64, bool EXPL, bool CTL, bool YREF = false, bool SEQY = false,
          bool WIDE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void als_solve_kernel(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ indices,
    const float *__restrict__ values, const int32_t *__restrict__ order, int64_t n_rows,
    const int32_t *__restrict__ row_slab, const float *__restrict__ other, int ld_other,
    float *__restrict__ this_, int ld_this, const float *__restrict__ otor_p,
    const float *__restrict__ slabs, float *__restrict__ row_delta, int *__restrict__ status,
    int k, float reg, TaskCtlDev ctl, const float *__restrict__ y_ref = nullptr,
    int chunk_rt = 0)
{
    __shared__ __attribute__((aligned(16))) float lds_flat[4 * hybrid_lds_floats<NT>()];
    als_solve_body<NT, IS64, EXPL, CTL, YREF, SEQY, WIDE>(indptr, indices, values, order, n_rows,
                                                    row_slab, other, ld_other, this_, ld_this,
                                                    otor_p, slabs, row_delta, status, k, reg, ctl,
                                                    y_ref, chunk_rt, (int64_t)blockIdx.x, lds_flat);
}

// ---- Woodbury row solve for rows with 17..64 entries at padded k = 128 / 256 -----------------
//
// Same identity as csrc/als_wb.hip (see there): x = sum_j (w_j - sqrt(v_j) u_j) z_j with
// S u = sqrt(v) o (S0 w), S = I + diag(sqrt v) S0 diag(sqrt v), S0 = [q_i . z_j] -- but S is up
// to 64 x 64 now: exactly the system the k = 64 hybrid solver above factors in accumulator
// tiles.  One wave per row; entry e = 16 t + c, lane (s, c) = (feature quarter s, slot c) holds
// the entries t = 0..3 of its slot.  Pass 1 streams the quarter's features four at a time and
// accumulates ALL 16 tiles of S0 (the lower ones only feed the row sums S0 w); `hybrid_solve<4>`
// solves; pass 2 re-reads z (L1/L2 hits) for x = sum_e g_e z_e with a 16-lane DPP butterfly.
template <int CTRL>
__device__ __forceinline__ float wb_dpp_add(float x)
{
    const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false);
    return x + __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float wb_row16_sum(float x)
{
    x = wb_dpp_add<0xB1>(x);   // quad_perm [1,0,3,2]
    x = wb_dpp_add<0x4E>(x);   // quad_perm [2,3,0,1]
    x = wb_dpp_add<0x141>(x);  // row_half_mirror
    x = wb_dpp_add<0x140>(x);  // row_mirror
    return x;
}

template <int KP, bool IS64>
__global__ __launch_bounds__(256) void als_wb64_kernel(
    const typename IndPtr<IS64>::type *__restrict__ indptr, const int32_t *__restrict__ indices,
    const float *__restrict__ values, const int32_t *__restrict__ order, int64_t n_tasks,
    const float *__restrict__ other, const float *__restrict__ z, float *__restrict__ this_,
    float *__restrict__ row_delta, int *__restrict__ status)
{
    constexpr int QF = KP / 4;  // features per quarter
    constexpr int NQ = QF / 4;  // chunks of 4 features
    __shared__ __attribute__((aligned(16))) float lds_all[4][hybrid_lds_floats<4>()];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int s = lane >> 4, c = lane & 15;
    const int64_t task = (int64_t)blockIdx.x * 4 + wave;
    if (task >= n_tasks) return;
    if (status[1] != 0) return;  // Z unavailable (OtOr not positive definite): dense fallback
    const int row = order[task];
    const int64_t beg = indptr[row], end = indptr[row + 1];
    const int n = (int)(end - beg);  // 17 .. 64 (any 1 .. 64 is handled)
    float *xrow = this_ + (int64_t)row * KP;
    float *lds = lds_all[wave];
    const int nte = __builtin_amdgcn_readfirstlane((n + 15) >> 4);  // entry tiles in use

    // this lane's entries: slot c of every tile (slots past the row end: zero weights)
    const float *mrow[4], *zrow[4];
    float w[4], sv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int el = 16 * t + c;
        const int64_t e = beg + (el < n ? el : n - 1);
        const int col = indices[e];
        const float v = el < n ? values[e] : 0.f;
        w[t] = el < n ? v + 1.0f : 0.f;
        sv[t] = __builtin_sqrtf(v);
        // Feature interleave (round 4): step q covers features 16 q .. 16 q + 15 and lane (s, c)
        // takes 4 s .. 4 s + 3 of them, so the four lanes of an entry slot read 64 CONTIGUOUS
        // bytes of the gathered row per step.  (Rounds 2-3 gave lane (s, c) the quarter
        // [64 s, 64 s + 64): 16 bytes per 128-byte line and step, each line revisited on 8
        // steps -- with 230 MB of rows in flight they did not survive in L2: FETCH_SIZE 164 GB per
        // cfg5 item half for 32 GB of rows, the kernel ran at 6.6 TB/s of HBM traffic.)  MFMA
        // step el then contracts features {16 q + el, + 4, + 8, + 12} on BOTH operands.
        mrow[t] = other + (int64_t)col * KP + 4 * s;
        zrow[t] = z + (int64_t)col * KP + 4 * s;
    }
    // pass 1: S0 tiles, acc[ti][tj] lane (s', c') register r = S0[16 ti + 4 s' + r][16 tj + c']
    f32x4 acc[4][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < NQ; ++q) {
        f32x4 mq[4], zq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            mq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            zq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < nte) {
                mq[t] = *reinterpret_cast<const f32x4 *>(mrow[t] + 16 * q);
                zq[t] = *reinterpret_cast<const f32x4 *>(zrow[t] + 16 * q);
            }
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
                if (ti < nte && tj < nte) {
#pragma unroll
                    for (int el = 0; el < 4; ++el)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            mq[ti][el], zq[tj][el], acc[ti][tj], 0, 0, 0);
                }
    }
    // S = I + diag(sv) S0 diag(sv) (upper tiles) and the right-hand side sv o (S0 w); rows with
    // at most 32 entries (round 4: most of the 17 .. 64 range) are a 32 x 32 system -- the k = 32
    // instance of the hybrid solver, a quarter of the factorisation work
    float b;
    float minpiv;
    auto build = [&](auto &G, auto ntc) {
        constexpr int NTS = decltype(ntc)::value;
#pragma unroll
        for (int ti = 0; ti < NTS; ++ti) {
            float svr[4], rhs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                svr[r] = __shfl(sv[ti], 4 * s + r, 64);  // sqrt(v) of row 16 ti + 4 s + r
                float r0 = 0.f;
#pragma unroll
                for (int tj = 0; tj < NTS; ++tj) r0 += wb_row16_sum(acc[ti][tj][r] * w[tj]);
                rhs[r] = svr[r] * r0;
            }
#pragma unroll
            for (int tj = ti; tj < NTS; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    G.t[tidx(ti, tj)][r] = svr[r] * sv[tj] * acc[ti][tj][r] +
                                           ((ti == tj && (4 * s + r) == c) ? 1.0f : 0.f);
            // rhs of row 16 ti + c for every lane: it sits in row group c >> 2, register c & 3
            float sel = rhs[0];
            sel = (c & 3) == 1 ? rhs[1] : sel;
            sel = (c & 3) == 2 ? rhs[2] : sel;
            sel = (c & 3) == 3 ? rhs[3] : sel;
            G.y[ti] = __shfl(sel, (c >> 2) * 16 + c, 64);
        }
    };
#ifdef LK_ALS_PHASES
    unsigned long long tmid_unused = 0;
#endif
    if (nte <= 2) {  // wave-uniform
        Gram<2> G;
        build(G, std::integral_constant<int, 2>{});
#ifdef LK_ALS_PHASES
        minpiv = hybrid_solve<2>(G, b, lds, &tmid_unused);
#else
        minpiv = hybrid_solve<2>(G, b, lds);
#endif
    } else {
        Gram<4> G;
        build(G, std::integral_constant<int, 4>{});
#ifdef LK_ALS_PHASES
        minpiv = hybrid_solve<4>(G, b, lds, &tmid_unused);
#else
        minpiv = hybrid_solve<4>(G, b, lds);
#endif
    }
    // b = u' of entry `lane`;  g_e = w_e - sv_e u'_e for this lane's four entries
    float g[4];
    bool bad = !(minpiv > 0.f);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        // (tiles past the row's entries -- and, for a 32 x 32 system, lanes the solver did not
        // define -- carry no weight)
        g[t] = t < nte ? w[t] - sv[t] * __shfl(b, 16 * t + c, 64) : 0.f;
        bad = bad || !(fabsf(g[t]) <= 3.0e38f);
    }
    if (__any(bad) && lane == 0) atomicCAS(status, 0, row + 1);
    // pass 2: x = sum_e g_e z_e
    float d2 = 0.f;
    for (int q = 0; q < NQ; ++q) {
        f32x4 a4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nte) {
                const f32x4 zq = *reinterpret_cast<const f32x4 *>(zrow[t] + 16 * q);
                a4.x = fmaf(g[t], zq.x, a4.x);
                a4.y = fmaf(g[t], zq.y, a4.y);
                a4.z = fmaf(g[t], zq.z, a4.z);
                a4.w = fmaf(g[t], zq.w, a4.w);
            }
        f32x4 xs;
        xs.x = wb_row16_sum(a4.x);
        xs.y = wb_row16_sum(a4.y);
        xs.z = wb_row16_sum(a4.z);
        xs.w = wb_row16_sum(a4.w);
        if (c == 0) {
            f32x4 *dst = reinterpret_cast<f32x4 *>(xrow + 4 * s + 16 * q);
            const f32x4 old = *dst;
            *dst = xs;
            const f32x4 d = xs - old;
            d2 += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
    }
    d2 = wave_sum(d2);
    if (lane == 0) row_delta[row] = d2;
}

// rows [t0, t1) of the plan order (17 .. 64 entries each)
int als_wb64_launch(const lk_als_plan *p, const void *indptr, int is64, const int32_t *indices,
                    const float *values, int64_t t0, int64_t t1, float *this_,
                    const float *other, const float *z, float *row_delta, int *status,
                    hipStream_t st)
{
    const int64_t n = t1 - t0;
    if (n <= 0) return LK_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
#define LK_WB64(KPV, IS)                                                                        \
    hipLaunchKernelGGL((als_wb64_kernel<KPV, IS>), grid, block, 0, st,                          \
                       static_cast<const typename IndPtr<IS>::type *>(indptr), indices, values, \
                       p->d_order + t0, n, other, z, this_, row_delta, status)
    if (p->KP == 256) {
        if (is64)
            LK_WB64(256, true);
        else
            LK_WB64(256, false);
    } else if (p->KP == 128) {
        if (is64)
            LK_WB64(128, true);
        else
            LK_WB64(128, false);
    } else {
        set_error("Woodbury row solve: unsupported padded embedding size %d", p->KP);
        return LK_E_INVALID;
    }
#undef LK_WB64
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// OtOr [k x k] -> primed [KP x KP] with identity on the pad features.
template <int NT>
__global__ void als_prep_otor_kernel(const float *__restrict__ otor, int ld_otor, int k,
                                     float *__restrict__ otor_p)
{
    constexpr int KP = NT * 16;
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= KP * KP) return;
    int pr = idx / KP, pc = idx % KP;
    int fr = (pr & 15) * NT + (pr >> 4), fc = (pc & 15) * NT + (pc >> 4);
    float v;
    if (fr < k && fc < k)
        v = otor ? otor[fr * ld_otor + fc] : 0.f;  // explicit mode: no OtOr term
    else
        v = (pr == pc) ? 1.0f : 0.0f;
    otor_p[idx] = v;
}

// deterministic two-stage sum of row deltas -> sqrt (the loops live in delta_reduce.h: the fused
// tail kernels of gramian.hip run the same ones)
__global__ void delta_partial_kernel(const float *__restrict__ row_delta, int64_t n,
                                     float *__restrict__ partial)
{
    __shared__ float sm[256];
    delta_partial_body(row_delta, n, (int)gridDim.x, (int)blockIdx.x, sm, partial);
}

__global__ void delta_final_kernel(const float *__restrict__ partial, int n,
                                   float *__restrict__ out)
{
    __shared__ float sm[256];
    delta_final_body(partial, n, sm, out);
}

constexpr int DELTA_BLOCKS = LK_DELTA_BLOCKS;

int launch_delta_reduce(const float *row_delta, int64_t n_rows, float *partial, float *out_frob,
                        hipStream_t st)
{
    hipLaunchKernelGGL(delta_partial_kernel, dim3(DELTA_BLOCKS), dim3(256), 0, st, row_delta,
                       n_rows, partial);
    hipLaunchKernelGGL(delta_final_kernel, dim3(1), dim3(256), 0, st, partial, DELTA_BLOCKS,
                       out_frob);
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// One half-epoch in the parts its schedule is made of (launch_chol below runs them one after the
// other; als_chol_epoch interleaves the two halves of an epoch):
//   prep   status word zeroed, OtOr primed and padded into the workspace (launch stream)
//   front  reads only `other`: chunk kernel, reference-order chains, ordered slab sums
//   solve  reads the primed OtOr: the short rows on the launch stream, the long rows (the rows of
//          the chains) on the side stream right behind their slab sums, then the join
//   tail   the delta reduction (launch_delta_reduce), or gramian_tail (gramian.hip) in an epoch
template <int NT, bool IS64, bool EXPL>
struct CholKind {};  // the kernels' template arguments as a value (chol_dispatch)

struct CholHalf {
    const lk_als_plan *p;
    const void *indptr;
    bool is64;  // width of the CSR offsets at `indptr`
    const int32_t *indices;
    const float *values;
    int64_t n_rows;
    int k;
    float *this_;
    int ld_this;
    const float *other;
    int ld_other;
    char *ws;
    float reg;
    hipStream_t st;
    // set by the front
    hipStream_t sr = nullptr;  // the stream of the chains (st: no fork)
    int64_t n_solve = 0, n_y = 0;
    float *yref = nullptr;
    bool tm = false;
    bool forked = false;
    // rows of `other` (the gathered table); negative: unknown
    int64_t n_cols = -1;

    // 64-bit gather addresses in the k = 64 Gram loops (dma_issue): unless the table is known to
    // be smaller than 4 GiB, so that every byte offset into it fits 32 bits
    bool wide() const
    {
        return n_cols < 0 || (uint64_t)n_cols * (uint64_t)ld_other * sizeof(float) >= (1ull << 32);
    }

    int *status() const { return reinterpret_cast<int *>(ws + p->off_status); }
    float *otor_p() const { return reinterpret_cast<float *>(ws + p->off_otor); }
    float *row_delta() const { return reinterpret_cast<float *>(ws + p->off_delta); }
    float *partial() const { return reinterpret_cast<float *>(ws + p->off_partial); }
    float *slabs() const { return reinterpret_cast<float *>(ws + p->off_slabs); }
    // every join happens on every path: whoever leaves between fork and join (an error return)
    // still makes the launch stream wait for the side stream -- the caller frees the workspaces
    ~CholHalf()
    {
        if (forked) (void)plan_join_rhs(p, st);
    }
};

template <int NT, bool IS64, bool EXPL>
static int chol_prep(CholHalf &h, CholKind<NT, IS64, EXPL>, const float *otor, int ld_otor)
{
    constexpr int KP = NT * 16;
    const lk_als_plan *p = h.p;
    LK_REQUIRE(!p->ref_order || (p->d_yref && !p->ctl),
               "a reference-order ALS plan needs its rhs workspace (lk_als_plan_set_rhs_workspace) "
               "and no task-control block");
    LK_HIP_CHECK(hipMemsetAsync(h.status(), 0, 64, h.st));
    if (p->ctl) {
        // a cancelled half-epoch leaves the rows not yet started untouched; their deltas
        // must not be garbage in the (discarded) sum
        LK_HIP_CHECK(hipMemsetAsync(h.row_delta(), 0, (size_t)h.n_rows * sizeof(float), h.st));
        int rc = ctl_begin(p->ctl, h.n_rows, h.n_rows, h.st);
        if (rc != LK_OK) return rc;
    }
    hipLaunchKernelGGL(als_prep_otor_kernel<NT>, dim3((KP * KP + 255) / 256), dim3(256), 0, h.st,
                       otor, ld_otor, h.k, h.otor_p());
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

template <int NT, bool IS64, bool EXPL>
static int chol_front(CholHalf &h, CholKind<NT, IS64, EXPL>)
{
    const lk_als_plan *p = h.p;
    hipStream_t st = h.st;
    float *slabs = h.slabs();
    h.tm = p->timing && p->timing_n < lk_als_plan::TIMING_RING;
    if (h.tm) LK_HIP_CHECK(hipEventRecord(p->ev[p->timing_n][0], st));
    // (CG hybrid: only the chunked rows, the first dense_limit tasks of the order)
    h.n_solve = p->dense_limit >= 0 && p->dense_limit < h.n_rows ? p->dense_limit : h.n_rows;
    // rows whose right-hand side comes from the reference-order chain (als_rhs.hip): the long
    // rows (the first n_long tasks) of a hybrid plan, every row of a strict reference-order plan
    h.yref = p->hybrid ? reinterpret_cast<float *>(h.ws + p->off_yref)
                       : (p->ctl ? nullptr : p->d_yref);
    h.n_y = !h.yref ? 0 : (p->hybrid ? std::min<int64_t>(p->n_long, h.n_solve) : h.n_solve);
    // The chains run on the plan's second stream, beside the chunk kernel and the solve of
    // the other rows; only the (small) solve launch of the long rows waits for them.  They are
    // ENQUEUED BEHIND the chunk kernel (the fork point is in front of it): the chain kernel is
    // LDS-heavy and latency-bound; enqueued first it takes every CU's LDS for its first round
    // of workgroups and the MFMA-bound chunk kernel waits (measured: +0.25 ms per cfg2 item
    // half); enqueued second it trickles in as chunk workgroups retire and does most of its
    // work under the solve of the short rows.
    h.sr = st;
    if (h.n_y > 0) {
        int rc = plan_fork_rhs(p, st, &h.sr);
        if (rc != LK_OK) return rc;
        h.forked = h.sr != st;
    }
    // every row that owns slabs (the first n_long tasks) takes its y from the chains: the chunk
    // kernel forms no right-hand side, the slabs' y words stay unwritten and nobody reads them
    // (the YREF solve skips them, the slab sums below stop in front of them)
    const bool chunk_y = !(h.yref != nullptr && h.n_y >= p->n_long);
    constexpr bool CAN_WIDE = NT == 4;  // (only the k = 64 loops gather by DMA)
    const bool wide = CAN_WIDE && h.wide();
    if (p->n_chunks > 0) {
#define LK_CHUNK_LAUNCH(WITHY)                                                                  \
    if (wide)                                                                                  \
        LK_CHUNK_LAUNCH_W(WITHY, CAN_WIDE);                                                    \
    else                                                                                       \
        LK_CHUNK_LAUNCH_W(WITHY, false)
#define LK_CHUNK_LAUNCH_W(WITHY, WIDEV)                                                         \
    hipLaunchKernelGGL((als_chunk_kernel<NT, EXPL, WITHY, WIDEV>),                             \
                       dim3((unsigned)((p->n_chunks + 3) / 4)), dim3(256), 0, st, h.indices,   \
                       h.values, p->d_chunk_beg, p->d_chunk_len, p->n_chunks, h.other,         \
                       h.ld_other, slabs, p->d_chunk_slab, p->unit > p->chunk ? (int)p->chunk : 0)
        if (chunk_y) {
            LK_CHUNK_LAUNCH(true);
        } else {
            LK_CHUNK_LAUNCH(false);
        }
#undef LK_CHUNK_LAUNCH
#undef LK_CHUNK_LAUNCH_W
    }
    if (h.n_y > 0) {
        int rc = launch_rhs_reference(p, h.indptr, IS64 ? 1 : 0, h.indices, h.values, p->d_order,
                                      h.n_y, h.other, EXPL, h.yref, h.sr);
        if (rc != LK_OK) return rc;
    }
    if (p->n_chunks > 0) {
        // the ordered slab sums of reference-order rows are pure HBM streaming: on the second
        // stream (behind the chains) they run under the solve of the rows that need no slabs
        hipStream_t sg = st;
        if (h.forked) {
            int rc = plan_rhs_wait_main(p, st);
            if (rc != LK_OK) return rc;
            sg = h.sr;
        }
        int rc = launch_slab_group_reduce(p, slabs, slab_floats<NT>(), sg,
                                          chunk_y ? 0 : (size_t)als_tiles(NT) * 256);
        if (rc != LK_OK) return rc;
    }
    if (h.tm) LK_HIP_CHECK(hipEventRecord(p->ev[p->timing_n][1], st));
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// `otor_ready` (may be null): an event behind which the primed OtOr and the status word of the
// workspace are valid; both streams of the solve wait for it
template <int NT, bool IS64, bool EXPL>
static int chol_solve(CholHalf &h, CholKind<NT, IS64, EXPL>, hipEvent_t otor_ready)
{
    const lk_als_plan *p = h.p;
    hipStream_t st = h.st;
    using IT = typename IndPtr<IS64>::type;
    const IT *ip = static_cast<const IT *>(h.indptr);
    const int ref_chunk = (p->ref_order || p->hybrid) ? p->chunk : 0;
    const int64_t n_y = h.n_y, n_solve = h.n_solve;
    float *yref = h.yref;
    constexpr bool CAN_WIDE = NT == 4;
    const bool wide = CAN_WIDE && h.wide();
    if (otor_ready) LK_HIP_CHECK(hipStreamWaitEvent(st, otor_ready, 0));
#define LK_SOLVE_LAUNCH(CTLV, YREFV, T0, NTASKS, YPTR, STREAM)                                \
    LK_SOLVE_LAUNCH_S(CTLV, YREFV, false, T0, NTASKS, YPTR, STREAM)
#define LK_SOLVE_LAUNCH_S(CTLV, YREFV, SEQV, T0, NTASKS, YPTR, STREAM)                        \
    do {                                                                                       \
        if (wide)                                                                              \
            LK_SOLVE_LAUNCH_W(CTLV, YREFV, SEQV, CAN_WIDE, T0, NTASKS, YPTR, STREAM);          \
        else                                                                                   \
            LK_SOLVE_LAUNCH_W(CTLV, YREFV, SEQV, false, T0, NTASKS, YPTR, STREAM);             \
    } while (0)
#define LK_SOLVE_LAUNCH_W(CTLV, YREFV, SEQV, WIDEV, T0, NTASKS, YPTR, STREAM)                 \
    hipLaunchKernelGGL((als_solve_kernel<NT, IS64, EXPL, CTLV, YREFV, SEQV, WIDEV>),           \
                       dim3((unsigned)(((NTASKS) + 3) / 4)), dim3(256), 0, (STREAM), ip,       \
                       h.indices, h.values, p->d_order + (T0), (NTASKS), p->d_row_slab,        \
                       h.other, h.ld_other, h.this_, h.ld_this, h.otor_p(), h.slabs(),         \
                       h.row_delta(), h.status(), h.k, h.reg,                                  \
                       (CTLV) ? p->ctl->dev() : TaskCtlDev{}, (YPTR), ref_chunk)
    // the rows that take their own right-hand side first (longest-first inside the launch) ...
    // (hybrid / reference-order plans: these rows form y in the reference's order inside
    // their Gram loop -- SEQY; the accurate mode keeps the four-slot sums)
    const bool seqy = p->hybrid || p->ref_order;
    if (n_solve > n_y) {
        if (p->ctl) {
            if (seqy)
                LK_SOLVE_LAUNCH_S(true, false, true, n_y, n_solve - n_y, nullptr, st);
            else
                LK_SOLVE_LAUNCH(true, false, n_y, n_solve - n_y, nullptr, st);
        } else {
            if (seqy)
                LK_SOLVE_LAUNCH_S(false, false, true, n_y, n_solve - n_y, nullptr, st);
            else
                LK_SOLVE_LAUNCH(false, false, n_y, n_solve - n_y, nullptr, st);
        }
    }
    // ... and the rows of the chains (hybrid plans: the long rows -- one slab + one solve each).
    // Their launch is less than a round of workgroups and its inputs are complete on the side
    // stream long before the short rows are through: it goes there, right behind the slab sums,
    // and the launch stream joins once.  (With a task-control block the launch keeps its place
    // behind the join: the progress count then still ends with the long rows.)
    if (n_y > 0) {
        if (p->ctl) {
            h.forked = false;
            int rc = plan_join_rhs(p, st);
            if (rc != LK_OK) return rc;
            LK_SOLVE_LAUNCH(true, true, 0, n_y, yref, st);
        } else {
            if (otor_ready && h.sr != st) LK_HIP_CHECK(hipStreamWaitEvent(h.sr, otor_ready, 0));
            LK_SOLVE_LAUNCH(false, true, 0, n_y, yref, h.sr);
            h.forked = false;
            int rc = plan_join_rhs(p, st);
            if (rc != LK_OK) return rc;
        }
    }
#undef LK_SOLVE_LAUNCH
#undef LK_SOLVE_LAUNCH_S
#undef LK_SOLVE_LAUNCH_W
    if (h.tm) {
        LK_HIP_CHECK(hipEventRecord(p->ev[p->timing_n][2], st));
        p->timing_n++;
    }
    LK_HIP_CHECK(hipGetLastError());
    return LK_OK;
}

// the phase `f` for the half's NT / offset width / model: f(CholKind<NT, IS64, EXPL>{})
template <class F>
static int chol_dispatch(const CholHalf &h, bool expl, F &&f)
{
    auto by_model = [&](auto nt, auto wide) {
        constexpr int NT = decltype(nt)::value;
        constexpr bool IS64 = decltype(wide)::value;
        return expl ? f(CholKind<NT, IS64, true>{}) : f(CholKind<NT, IS64, false>{});
    };
    auto by_width = [&](auto nt) {
        return h.is64 ? by_model(nt, std::true_type{}) : by_model(nt, std::false_type{});
    };
    switch (h.p->NT) {
        case 1: return by_width(std::integral_constant<int, 1>{});
        case 2: return by_width(std::integral_constant<int, 2>{});
        case 4: return by_width(std::integral_constant<int, 4>{});
    }
    set_error("%s: no Cholesky kernel for padded k=%d",
              expl ? "lk_als_explicit_half_epoch" : "lk_als_implicit_half_epoch", h.p->KP);
    return LK_E_INVALID;
}

static int half_prep(CholHalf &h, bool expl, const float *otor, int ld_otor)
{
    return chol_dispatch(h, expl, [&](auto kind) { return chol_prep(h, kind, otor, ld_otor); });
}

static int half_front(CholHalf &h, bool expl)
{
    return chol_dispatch(h, expl, [&](auto kind) { return chol_front(h, kind); });
}

static int half_solve(CholHalf &h, bool expl, hipEvent_t otor_ready)
{
    return chol_dispatch(h, expl, [&](auto kind) { return chol_solve(h, kind, otor_ready); });
}

size_t als_chol_slab_floats(int NT) { return (size_t)(als_tiles(NT) * 4 + NT) * 64; }

// Exact half-epoch for padded k <= 64 (dispatch target of lk_als_implicit_half_epoch /
// lk_als_explicit_half_epoch); `otor` null = explicit model.  `n_cols`: rows of `other`, or
// negative if the caller does not know (the gathers then use 64-bit addresses).
int als_chol_half_epoch(const lk_als_plan *p, const void *indptr, int is64, const int32_t *indices,
                        const float *values, int64_t n_rows, int64_t n_cols, int k, float *this_,
                        int ld_this, const float *other, int ld_other, const float *otor,
                        int ld_otor, char *ws, float *out_frob, hipStream_t st, bool expl, float reg)
{
    CholHalf h{p, indptr, is64 != 0, indices, values, n_rows, k, this_, ld_this, other, ld_other, ws, reg, st};
    h.n_cols = n_cols;
    int rc = half_prep(h, expl, otor, ld_otor);
    if (rc == LK_OK) rc = half_front(h, expl);
    if (rc == LK_OK) rc = half_solve(h, expl, nullptr);
    if (rc != LK_OK) return rc;
    return launch_delta_reduce(h.row_delta(), n_rows, h.partial(), out_frob, st);
}

// One implicit epoch, both halves in one schedule (lk_als_implicit_epoch, include/lkamd.h):
//
//   st:      prep U, front U (chunk U) -> solve-short U -> join side_U -> front I (chunk I)
//            -> wait E_tailU -> solve-short I -> join side_I -> tail I
//   side_U:  chains U -> slab sums U -> solve-long U ... then, behind the join point:
//            tail U (delta U, Gramian(P), primed OtOr + status word of plan I) -> E_tailU
//   side_I:  chains I -> slab sums I -> wait E_tailU -> solve-long I
//
// Front I reads only P: it does not wait for tail U, which runs under the item half's chunk
// kernel; only the solve launches of the item half do.  Stream order only: no graph capture,
// no flags between workgroups.  When the call returns, `st` holds everything.
int als_chol_epoch(const lk_als_plan *pu, const lk_als_plan *pi, const void *u_indptr,
                   const int32_t *u_indices, const float *u_values, const void *i_indptr,
                   const int32_t *i_indices, const float *i_values, float *P, float *Q,
                   float *qtq, int ld_qtq, float user_reg, float *ptp, int ld_ptp, float item_reg,
                   char *ws_u, char *ws_i, float *gram_ws, float *out_delta, hipStream_t st)
{
    const int k = pu->k, KP = pu->KP;
    CholHalf hu{pu, u_indptr, pu->is64 != 0, u_indices, u_values, pu->n_rows, k, P, KP, Q, KP, ws_u, 0.f, st};
    CholHalf hi{pi, i_indptr, pi->is64 != 0, i_indices, i_values, pi->n_rows, k, Q, KP, P, KP, ws_i, 0.f, st};
    hu.n_cols = pi->n_rows;  // (each half gathers the rows the other one solves)
    hi.n_cols = pu->n_rows;
    int rc = half_prep(hu, false, qtq, ld_qtq);
    if (rc == LK_OK) rc = half_front(hu, false);
    if (rc == LK_OK) rc = half_solve(hu, false, nullptr);
    if (rc != LK_OK) return rc;
    // tail U on the user plan's side stream (idle by now), behind everything `st` holds
    hipStream_t tu = st;
    rc = plan_fork_rhs(pu, st, &tu);
    if (rc != LK_OK) return rc;
    hu.forked = tu != st;  // (joined through E_tailU below; by the destructor on an error)
    rc = gramian_tail(P, pu->n_rows, k, KP, item_reg, ptp, ld_ptp, gram_ws, hu.row_delta(),
                      hu.partial(), out_delta, hi.otor_p(), hi.status(), tu);
    if (rc != LK_OK) return rc;
    hipEvent_t tail_u = nullptr;
    if (tu != st) {
        LK_HIP_CHECK(hipEventRecord(pu->ev_tail_rhs, tu));
        tail_u = pu->ev_tail_rhs;
    }
    rc = half_front(hi, false);
    if (rc == LK_OK) rc = half_solve(hi, false, tail_u);
    if (rc != LK_OK) return rc;
    hu.forked = false;  // st has waited for E_tailU in half_solve
    return gramian_tail(Q, pi->n_rows, k, KP, user_reg, qtq, ld_qtq, gram_ws, hi.row_delta(),
                        hi.partial(), out_delta + 1, nullptr, nullptr, st);
}

}  // namespace lk

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

#ifdef LK_ALS_PHASES
extern "C" int lk_als_phase_set(void *d_buf)
{
    LK_HIP_CHECK(hipDeviceSynchronize());
    LK_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(lk::lk_als_phase_buf), &d_buf, sizeof(void *)));
    return LK_OK;
}
#endif
