"""
The lane-level NumPy models of the ALS Cholesky kernels (tools/emul) stay runnable: they are
how the index arithmetic of csrc/als_chol.hip (accumulator-tile layout, L image, permlane
transposition) is checked without a GPU.  Likewise the LDS placement of the DMA-staged top-K
filter kernel (csrc/topk.hip::score_filter64_kernel), the per-target accumulator of the kNN
scoring kernels (csrc/iknn_score.hip: rounds, rank sort, BinaryHeap replay, in-place heapify)
against the C oracle, the folded 8-way reduction of the CG kernel (csrc/als_cg.hip), the
wave-per-row selection of the fused top-N path (csrc/topk.hip::cand_select_wave_kernel), and one
pass of the stable radix sort (csrc/radix_sort.h: histogram, scan with its carry, scatter ranks).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools" / "emul"))


@pytest.mark.parametrize("model", ["hybrid_chol", "panel_chol"])
@pytest.mark.parametrize("kp", [16, 64])
def test_lane_level_model_solves(model, kp):
    mod = __import__(model)
    rng = np.random.default_rng(kp)
    m = rng.standard_normal((kp + 30, kp)).astype(np.float32)
    a = (m.T @ m + 0.5 * np.eye(kp)).astype(np.float32)
    y = rng.standard_normal(kp).astype(np.float32)
    x, minpiv = mod.solve(a, y)
    ref = np.linalg.solve(a.astype(np.float64), y.astype(np.float64))
    assert minpiv > 0
    assert np.linalg.norm(x - ref) <= 1e-5 * np.linalg.norm(ref)


def test_permlane_transposition_model():
    import hybrid_chol as h

    x = [np.arange(64, dtype=np.float32) + 100 * r for r in range(4)]
    y = h.transpose4(x)
    lanes = np.arange(64)
    for r in range(4):
        # y[r] at row group g = x[g] at row group r
        want = 100 * (lanes >> 4) + (16 * r + (lanes & 15))
        assert np.array_equal(y[r], want.astype(np.float32))


def test_filter64_lds_layout_model():
    "every operand fetch of score_filter64_kernel reads what the LDS DMA placed; 2-way banks"
    import filter64_layout as f

    assert f.check() == (2, 2)


@pytest.mark.parametrize("max_nbrs", [1, 2, 5, 20])
@pytest.mark.parametrize("explicit", [True, False])
def test_knn_accumulator_model_matches_the_oracle(oracle, max_nbrs, explicit):
    """csrc/iknn_score.hip per target, modelled in tools/emul/knn_accum.py: rounds of history rows
    with the hits arriving in arbitrary order, rank sort, vector -> heap (staged pushes as in the
    list kernel, reverse + sift-up in place as in the slot kernel), std's BinaryHeap push / pop,
    sequential unfused sums -- against the C restatement of accum.rs, bit for bit, on inputs
    FULL of equal weights (where the eviction order matters)."""
    import scipy.sparse as sps

    import knn_accum as ka

    rng = np.random.default_rng(100 * max_nbrs + explicit)
    for trial in range(40):
        n_hist = int(rng.integers(0, 90))
        hit = rng.random(n_hist) < 0.7
        # few distinct weights: ties everywhere, at the boundary too
        weights = rng.choice(np.array([0.125, 0.25, 0.25, 0.5, 0.3, 0.7], np.float32), n_hist)
        values = rng.standard_normal(n_hist).astype(np.float32)
        target = n_hist  # one more item: the target
        rows = np.flatnonzero(hit)
        sims = sps.csr_array((weights[rows], (rows, np.full(len(rows), target))),
                             shape=(n_hist + 1, n_hist + 1), dtype=np.float32)
        want_s, want_c = oracle.iknn_score(sims, np.arange(n_hist, dtype=np.int32),
                                           values if explicit else None,
                                           np.array([target], np.int32), max_nbrs, 1)
        hits = [(int(r), weights[r], values[r] if explicit else np.float32(0)) for r in rows]
        for in_place in (False, True):
            for cap in (256, 16, 7):
                got_s, got_c = ka.score_target(hits, max_nbrs, 1, explicit, cap=cap,
                                               in_place=in_place, rng=rng)
                assert got_c == int(want_c[0]), (trial, in_place, cap)
                if np.isnan(want_s[0]):
                    assert np.isnan(got_s)
                else:
                    assert np.float32(got_s).view(np.uint32) == want_s[:1].view(np.uint32)[0], \
                        (trial, in_place, cap, got_s, want_s[0])


def test_cg_reduce8_model():
    "csrc/als_cg.hip::cg_reduce8: lane L ends with the wave-wide sum of item CG_REV3(L & 7)"
    import knn_accum as ka

    rng = np.random.default_rng(8)
    a = rng.standard_normal((64, 8))
    d = ka.cg_reduce8(a)
    tot = a.sum(axis=0)
    for lane in range(64):
        assert abs(d[lane] - tot[ka.cg_rev3(lane & 7)]) < 1e-12
    assert sorted(ka.cg_rev3(j) for j in range(8)) == list(range(8))
    assert all(ka.cg_rev3(ka.cg_rev3(j)) == j for j in range(8))


def test_inverted_diagonal_blocks_are_as_accurate_as_substitution():
    """tools/emul/blk_diaginv.py -- the numerics of the next k = 128 / 256 row solve:
    a blocked float32 Cholesky with INVERTED 16 x 16 diagonal blocks (panel rows and both
    triangular solves as small GEMMs) against the substitution form the kernel uses today."""
    import blk_diaginv as b

    rng = np.random.default_rng(3)
    rel = lambda a, c: float(np.linalg.norm(a - c) / np.linalg.norm(c))  # noqa: E731
    for k, cond in ((48, 1e2), (128, 1e3), (128, 1e5)):
        q, _ = np.linalg.qr(rng.standard_normal((k, k)))
        a = (q * np.geomspace(1.0, cond, k)) @ q.T
        y = rng.standard_normal(k)
        x64 = np.linalg.solve(a, y)
        es, ei = rel(b.solve_blocked(a, y, False), x64), rel(b.solve_blocked(a, y, True), x64)
        u = 2.0 ** -24
        assert es < 2 * cond * u and ei < 2 * cond * u, (k, cond, es, ei)
        assert ei < 3 * es + 1e-7, (k, cond, es, ei)


def test_wave_select_model_equals_a_sort():
    """hash of the candidates' items with struck exclusions, two-stage threshold search, ballot
    compaction, 128-key register network: the top n of what survives, in order"""
    import wave_select as w

    assert w.main(trials=120) > 32  # the index-half search ran (more than 128 equal scores)


# ---- csrc/radix_sort.h ----------------------------------------------------------------------------
def _digits(kind, n, mask, rng):
    i = np.arange(n, dtype=np.uint64)
    top = np.uint64(mask)
    if kind == "all 0":
        return np.zeros(n, np.uint64)
    if kind == "all top":
        return np.full(n, top, np.uint64)
    if kind == "two alternating":
        return np.where(i % np.uint64(2) == 0, top, np.uint64(min(3, mask - 1)))
    if kind == "uniform":
        return rng.integers(0, mask + 1, n, dtype=np.uint64)
    if kind == "ascending":
        return (i * np.uint64(mask + 1)) // np.uint64(n)
    assert kind == "descending"
    return top - (i * np.uint64(mask + 1)) // np.uint64(n)


RADIX_DISTRIBUTIONS = ["all 0", "all top", "two alternating", "uniform", "ascending", "descending"]


@pytest.mark.parametrize("mask", [255, 1])
@pytest.mark.parametrize("tile_n", [1, 63, 64, 65, 4095, 4096])
def test_radix_scatter_model_is_a_stable_pass(tile_n, mask):
    """tools/emul/radix_scatter.py: the eight-ballot peers mask and rank, the uint16 per-(chunk,
    digit) table and its running offsets, the four-per-lane wave scan of tile_start, the uint16 pos,
    the digit-major reorder and the destination from goff -- one pass over a single tile (and over
    that tile behind a full one) equals a stable sort by the digit, for every digit distribution;
    mask 1 is the 1-bit last digit of a 33- or 41-bit key."""
    import radix_scatter as rs

    rng = np.random.default_rng(1000 * tile_n + mask)
    shift = 16
    for kind in RADIX_DISTRIBUTIONS:
        for n in (tile_n, rs.TILE + tile_n):
            dig = _digits(kind, n, mask, rng)
            assert int(dig.max()) <= mask
            if kind == "all top":
                assert (dig == mask).all()
            if kind == "two alternating":
                assert len(np.unique(dig)) == min(2, n)
            # bits around the digit are noise the pass must ignore; equal digits everywhere
            noise = rng.integers(0, 1 << 16, n, dtype=np.uint64)
            high = rng.integers(0, 1 << 20, n, dtype=np.uint64) << np.uint64(shift + 8)
            keys = noise | (dig << np.uint64(shift)) | (high if mask == 255 else np.uint64(0))
            vals = np.arange(n, dtype=np.uint32)
            assert np.array_equal(rs.digit_of(keys, shift, mask), dig.astype(np.uint32))
            gk, gv = rs.radix_pass(keys, vals, shift, mask)
            order = np.argsort(dig, kind="stable")
            assert np.array_equal(gv, vals[order]), (kind, n)
            assert np.array_equal(gk, keys[order]), (kind, n)
            k32 = (keys & np.uint64(0xffffffff)).astype(np.uint32)  # the <uint32, uint64> pairs
            gk, gv = rs.radix_pass(k32, vals.astype(np.uint64), shift, mask)
            assert np.array_equal(gv, vals[order]) and np.array_equal(gk, k32[order]), (kind, n)


@pytest.mark.parametrize("n_tiles", [1, 2, 256, 257])
def test_radix_scan_model_trips_and_carry(n_tiles):
    """rs_hist / rs_rowsum / rs_scan: where tile i's keys of digit d start = the totals of the
    smaller digits + digit d's counts in the tiles before i; 257 tiles take a second 256-wide trip
    whose first entry is the carry of the first."""
    import radix_scatter as rs

    rng = np.random.default_rng(n_tiles)
    hist = rng.integers(0, rs.TILE + 1, (rs.RADIX, n_tiles)).astype(np.uint64)
    hist[rng.random(hist.shape) < 0.3] = 0
    hist[7, :] = rs.TILE  # a digit every tile is full of
    total = rs.rowsum_model(hist)
    assert np.array_equal(total, hist.sum(axis=1))
    offs, trips = rs.scan_model(hist, total)
    assert trips == (n_tiles + 255) // 256 == (2 if n_tiles == 257 else 1)
    before = np.concatenate([[0], np.cumsum(total)[:-1]]).astype(np.uint64)
    want = before[:, None] + np.cumsum(hist, axis=1) - hist
    assert np.array_equal(offs, want)
    if n_tiles == 257:
        assert offs[7, 256] == before[7] + 256 * rs.TILE  # what the carry brings over
    # ... and the histogram itself, on keys that end inside the last tile
    n = min(n_tiles, 3) * rs.TILE - 5
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    h = rs.hist_model(keys, 8, 255)
    assert h.shape == (rs.RADIX, rs.tiles_of(n))
    for tile in range(h.shape[1]):
        d = rs.digit_of(keys[tile * rs.TILE:(tile + 1) * rs.TILE], 8, 255)
        assert np.array_equal(h[:, tile], np.bincount(d, minlength=rs.RADIX))


def test_radix_pass_model_across_257_tiles():
    "one whole modelled pass whose scan makes the second trip: 257 tiles, the last holding one key"
    import radix_scatter as rs

    rng = np.random.default_rng(257)
    n = 256 * rs.TILE + 1
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[: rs.TILE] = 0x00AB0000  # a full tile in which every key has the same digit
    vals = np.arange(n, dtype=np.uint32)
    assert rs.tiles_of(n) == 257
    gk, gv = rs.radix_pass(keys, vals, 16, 255)
    order = np.argsort(rs.digit_of(keys, 16, 255), kind="stable")
    assert np.array_equal(gv, vals[order]) and np.array_equal(gk, keys[order])


@pytest.mark.parametrize("end_bit", [32, 34, 41])
def test_radix_chained_passes_sort_64_bit_keys(end_bit):
    """radix_sort_pairs over (row << 32) | key as topn_sort builds them: 4, 5 and 6 passes, the last
    digit 8, 2 and 1 bits wide, the ping-pong ending in the out pair; equal keys keep their order"""
    import radix_scatter as rs

    rng = np.random.default_rng(end_bit)
    n = 2 * rs.TILE + 77
    plan = rs.pass_plan(0, end_bit)
    assert len(plan) == {32: 4, 34: 5, 41: 6}[end_bit]
    assert plan[-1][1] == {32: 255, 34: 3, 41: 1}[end_bit] and plan[-1][2]
    assert plan[0][2] == (len(plan) % 2 == 1)  # an even count: the first pass goes to the tmp pair
    rows = np.sort(rng.integers(0, 1 << (end_bit - 32), n, dtype=np.uint64)) if end_bit > 32 \
        else np.zeros(n, np.uint64)
    low = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    low[rng.random(n) < 0.5] = 0xFFFFFFFF - 0x3F800000  # heavy ties
    keys = (rows << np.uint64(32)) | low
    vals = rng.permutation(n).astype(np.uint32)
    assert n - len(np.unique(keys)) > n // 4 and int(keys.max()) < (1 << end_bit)
    gk, gv = rs.radix_sort_pairs(keys, vals, 0, end_bit)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(gk, keys[order]) and np.array_equal(gv, vals[order])


def test_radix_scatter_model_self_check():
    import radix_scatter as rs

    rs.main()
