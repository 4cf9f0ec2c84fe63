"""CPU: the NumPy restatement of the fused top-N path's stage 1 (``tests/topk_stage1_restatement.py``)
against independent statements of the same rules, and -- the condition that keeps the redo
assertion of ``tests/test_gpu_topk_widths.py`` from hiding anything -- for every input of that
module, the restatement alone yields exactly the redo rows the input was designed to have."""
import numpy as np
import pytest
from scipy.stats import binom

import topk_stage1_restatement as R
import topk_width_cases as C


def _rank_direct(n_items, n, keep, div=0):
    f = keep * R.fused_sample_items(n_items, n, div) / n_items
    for r in range(1, n):
        if binom.sf(r - 1, n - 1, f) <= 1.0e-6:  # P[X >= r]
            return r
    return n


@pytest.mark.parametrize("n", [1, 2, 10, 20, 100, 128])
def test_tau_rank_is_the_binomial_tail(n):
    # the last two: the sample is the whole catalogue (f = 1: only r = n is certain)
    for n_items in (4099, 8191, 8192, 20000, 62423, 1000003, 16 * n, max(2, n)):
        for keep in (1.0, 255 / 256, 0.5, 127 / 256, 64 / 256):
            assert R.fused_tau_rank(n_items, n, keep) == _rank_direct(n_items, n, keep), (n_items, keep)
        assert R.fused_tau_rank(n_items, n, 0.5, exact=True) == n
    for div in (2, 16, 64):
        assert R.fused_tau_rank(62423, n, 1.0, div=div) == _rank_direct(62423, n, 1.0, div)
    assert R.fused_sample_items(16 * n, n) == 16 * n and R.fused_stride(max(2, n), n) == 1


def test_tau_rank_known_values():
    "the figures csrc/topk.hip quotes, and the small shape's rank table"
    assert R.fused_tau_rank(62423, 100) == 18  # "r = 18 for n = 100 at ML-25M's 1 / 22"
    assert [R.fused_tau_rank(4099, 10, (256 - d) / 256) for d in (0, 1, 128, 192)] == [7, 7, 6, 5]
    assert R.fused_tau_rank(4099, 1) == 1


@pytest.mark.parametrize("n", [1, 10, 100, 128])
def test_sample_geometry_against_brute_force(n):
    for n_items in (64 * n, 64 * n + 1, 4099, 8191, 8192, 20000, 62423, 100000):
        for div in (0, 2, 16, 64):
            d = div or 24
            # smallest multiple of 256 that is >= max(floor(I / d), 16 n), capped at I
            want = next(s for s in range(256, n_items + 512, 256) if s >= max(n_items // d, 16 * n))
            want = min(want, n_items)
            assert R.fused_sub_items(n_items, n, div) == want
            st = R.fused_stride(n_items, n, div)
            assert st == max(1, n_items // want)
            sample = [i for i in range(n_items) if i % st == 0]
            assert R.fused_sample_items(n_items, n, div) == len(sample)
            assert sample[-1] < n_items <= sample[-1] + st


def test_split_geometry_against_brute_force():
    for rows in (1, 130, 8192, 8500, 12000, 30000, 65535, 65536, 65666):
        for n_items in (1792, 2048, 4099, 20000):
            wgs, tiles = -(-rows // 128), -(-n_items // 256)
            want = 1
            if wgs < 512 and tiles >= 8:  # the most parts that keep the launch inside one round
                want = max([p for p in range(2, 65) if p * wgs <= 512 and 4 * p <= tiles], default=1)
            for kp in (32, 64, 128, 256):
                assert R.filter_parts(rows, n_items, kp) == want
                assert R.filter_parts(rows, n_items, kp, split=False) == 1
            assert R.filter_parts(rows, n_items, 96) == 1  # register-staged kernel: never split
    assert [R.filter_part_cap(p) for p in (1, 2, 4, 6, 8, 64)] == [2048, 2048, 1024, 768, 512, 512]


def test_small_shape_geometry():
    g = R.geometry(C.B0, C.I0, C.N0, 256)
    assert (g["stride"], g["n_sample"], g["parts"], g["part_cap"], g["batches"], g["overlap"]) == (
        16, 257, 4, 1024, 1, False)
    assert R.geometry(8192 + 130, C.I0, C.N0, 128, env_rows=8192)["batches"] == 2
    assert R.geometry(8192 + 130, C.I0, C.N0, 128, env_rows=8192)["parts"] == 1
    assert R.geometry(65536 + 130, C.I0, C.N0, 64)["overlap"]
    assert not R.geometry(65536, C.I0, C.N0, 64)["overlap"]  # the first size with rows_a < rows
    assert not R.geometry(65536 + 130, C.I0, C.N0, 64, overlap=False)["overlap"]
    assert not R.use_fused(C.B0, 8191, 128, 64, 1, 1) and R.use_fused(C.B0, 8192, 128, 64, 1, 1)
    assert not R.use_fused(C.B0, 20000, 129, 64, 1, 1)
    assert not R.use_fused(C.B0, C.I0, 10, 16, 1, 1) and not R.use_fused(C.B0, C.I0, 10, 320, 1, 1)


def test_thresholds_on_a_hand_made_row():
    "both variants on a row small enough to follow by hand (I = 4099, n = 10: r = 7)"
    s = np.zeros(C.I0, np.float32)
    s[::16] = -np.arange(257, dtype=np.float32)  # sample column j scores -j
    assert R.tau_cmax(s, [], C.I0, 10) == (-6.0, 0)  # classes 0 .. 6 hold the 7 best
    # panel variant: float4 classes {0..3}, {4..7}, ...: the 7th best class maximum is column 24's
    assert R.tau_panel(s, [], C.I0, 10) == (-24.0, 0)
    # column 0 excluded: class 0 is dirty and dropped (column 256 with it), rank r[1] = 7
    assert R.tau_cmax(s, [0], C.I0, 10) == (-7.0, 1)
    assert R.tau_panel(s, [0, 5, -16, 16 * 257], C.I0, 10) == (-24.0, 0)  # class 0: column 1 now
    # 129 dirty classes: undetermined, unless every dirty class is repaired (r = n = 10)
    ex = 16 * np.arange(129)
    assert R.tau_cmax(s, ex, C.I0, 10) == (R.UNDETERMINED, 129)
    # classes 1 .. 128 lose their only column, class 0 is repaired from column 256
    assert R.tau_cmax(s, ex, C.I0, 10, exact=True) == (-138.0, 129)  # the 10th of -129, -130, ...
    s[16 * 3] = np.nan
    assert R.tau_cmax(s, [], C.I0, 10) == (-7.0, 0)  # NaN is no score
    # the verdict: item i scores -i, so tau = -t lets items 0 .. t through
    s = -np.arange(C.I0, dtype=np.float32)
    v = R.row_verdict(s, [], 10, -99.0, 4)
    assert (v["redo"], v["count"], v["valid"], v["tier2"]) == (False, 100, 100, False)
    assert R.row_verdict(s, np.arange(90), 10, -99.0)["why"] is None
    assert R.row_verdict(s, [5, *range(91), -1, C.I0], 10, -99.0)["why"] == "threshold too high"
    assert R.row_verdict(s, [], 10, -1500.0, 4)["tier2"] and not R.row_verdict(s, [], 10, -1023.0)["tier2"]
    assert R.row_verdict(s, [], 10, -2047.0, 4)["why"] is None  # 2048 candidates, 512 per part
    assert R.row_verdict(s, [], 10, -2048.0, 4)["why"] == "list overflows"
    # every score 0: part 0 walks tiles 0, 4, 8, 12 and 16 -- 1027 candidates for 1024 places
    assert R.row_verdict(np.zeros(C.I0, np.float32), [], 10, 0.0, 4)["why"] == "a part overflows"
    assert R.row_verdict(np.zeros(C.I0, np.float32), [], 10, 0.0, 1)["why"] == "list overflows"
    assert R.row_verdict(s, np.arange(5, C.I0), 10, R.UNDETERMINED)["redo"] is True


@pytest.fixture(scope="module")
def small_cases():
    return {k: C.small_case(k) for k in C.WIDTHS}


def _check(p, redo, und):
    assert p["redo"] == sorted(redo), (p["redo"], p["counts"])
    assert p["undetermined"] == sorted(und)


@pytest.mark.parametrize("k", C.WIDTHS)
def test_designed_redo_rows_small(oracle, small_cases, k):
    case = small_cases[k]
    # the knife-edge rows: n valid candidates at the threshold of the right rank only
    s = oracle.score_dense(case["Q"], case["U"][C.ROW_KNIFE])
    ex = case["lists"][C.ROW_KNIFE_128]
    assert R.tau_cmax(s, [], C.I0, C.N0) == (10.0, 0) and R.tau_panel(s, ex, C.I0, C.N0) == (10.0, 0)
    assert R.tau_cmax(s, ex, C.I0, C.N0) == (100.0, 128)  # rank r[128] = 6
    assert [R.row_verdict(s, [], C.N0, t, 4)["why"] for t in (100.0, 10.0, 1.0)] == [
        "threshold too high", None, "list overflows"]
    assert R.row_verdict(s, [], C.N0, 10.0)["count"] == 12
    for stage1 in ("cmax", "panel"):
        for split in (True, False):
            p = C.predict(oracle, case, stage1=stage1, split=split)
            _check(p, *C.designed(stage1))
            assert p["geometry"]["parts"] == (4 if split else 1)
            assert all(b in p["tier2"] for b in C.ROWS_TIER2)
            assert {b: p["nd"][b] for b in C.ROWS_ND} == (C.ROWS_ND if stage1 == "cmax" else dict.fromkeys(C.ROWS_ND, 0))
        p = C.predict(oracle, case, stage1=stage1, exact=True, div=16)
        _check(p, *C.designed(stage1, exact=True))
        assert all(C.R.FUSED_LCAP < p["counts"][b] <= C.R.FUSED_CAP for b in C.ROWS_TIER2)


@pytest.mark.parametrize("k", [25, 100, 200])
def test_designed_redo_rows_non_finite(oracle, k):
    case = C.non_finite_case(k)
    for stage1 in ("cmax", "panel"):
        p = C.predict(oracle, case, stage1=stage1)
        _check(p, [], [])  # infinite thresholds (50 +inf sample scores) still leave n candidates
    s = oracle.score_dense(case["Q"], case["U"][case["B"] - 1])
    assert R.tau_cmax(s, [], case["I"], case["n"])[0] == np.inf and np.isnan(s).any()




@pytest.mark.parametrize("k", [128, 256])
def test_designed_redo_rows_batches(oracle, small_cases, k):
    case = C.expand(small_cases[k], 8192 + 130, C.BATCH_OVERRIDES)
    p = C.predict(oracle, case, env_rows=8192)
    assert (p["geometry"]["batches"], p["geometry"]["parts"]) == (2, 1)
    _check(p, C.designed("cmax")[0] + [8191, 8192], C.designed("cmax")[1])


@pytest.mark.parametrize("k", [64, 256])
def test_designed_redo_rows_overlap(oracle, small_cases, k):
    case = C.expand(small_cases[k], 65536 + 130, C.OVERLAP_OVERRIDES)
    for overlap in (True, False):
        p = C.predict(oracle, case, overlap=overlap)
        assert p["geometry"]["overlap"] == overlap and p["geometry"]["parts"] == 1
        _check(p, C.designed("cmax")[0] + [65534, 65537], C.designed("cmax")[1])
        assert {65535, 65536} <= set(p["tier2"])


@pytest.mark.parametrize("k", [64, 256])
@pytest.mark.parametrize("I,n", [(C.I0, 1), (8192, 128)])
def test_designed_redo_rows_n_edges(oracle, I, n, k):
    case = C.n_edge_case(k, I, n)
    p = C.predict(oracle, case)
    _check(p, [], [])
