"""
GPU: the fused top-N path of ``lk_score_topk`` at every padded feature width that reaches it
(32, 64, 128, 256 -- ``score_filter64_kernel`` and ``score_filter_slab_kernel<32 / 128 / 256>``,
split and unsplit), bit for bit against the oracle and the panel path -- and, through
``lk_score_topk_last_report``, WHICH rows the device redid through the panel path: exactly the
rows the restatement of stage 1 (``tests/topk_stage1_restatement.py``) predicts, so that a defect
in the threshold or the filter cannot hide behind the redo path.  The inputs come from
``tests/topk_width_cases.py``; ``tests/test_topk_stage1_host.py`` checks on the host that the
restatement predicts for each of them the redo rows it was designed to have.
"""
import numpy as np
import pytest
import torch

import topk_stage1_restatement as R
import topk_width_cases as C

pytestmark = pytest.mark.gpu

PANEL = "1000000000"  # LK_TOPK_FUSED_MIN_ITEMS that switches the fused path off
_cache = {}


def _small(k):
    if ("small", k) not in _cache:
        _cache["small", k] = C.small_case(k)
    return _cache["small", k]


def _scores(oracle, case, t):
    "exact scores of base row t (computed once per case and row)"
    base = case.get("base", case)
    memo = base.setdefault("_scores", {})
    if t not in memo:
        memo[t] = oracle.score_dense(base["Q"], base["U"][t])
    return memo[t]


def _want(oracle, case, b):
    "row b's list by the oracle: (score desc, index asc), exclusions as NaN, -1 / NaN padding"
    n, I = case["n"], case["I"]
    t = int(case["tmpl"][b]) if "tmpl" in case else b
    s = _scores(oracle, case, t).copy()
    e = np.asarray(case["lists"][b], dtype=np.int64)
    s[e[(e >= 0) & (e < I)]] = np.nan
    top = oracle.argsort_descending(s)[:n]
    idx = np.full(n, -1, np.int32)
    sc = np.full(n, np.nan, np.float32)
    idx[: len(top)] = top
    sc[: len(top)] = s[top]
    return idx, sc


def _env(monkeypatch, variant=("cmax", "wave"), **kw):
    monkeypatch.setenv("LK_TOPK_STAGE1", variant[0])
    monkeypatch.setenv("LK_TOPK_SELECT", variant[1])
    monkeypatch.setenv("LK_TOPK_FUSED_MIN_USERS", "1")
    monkeypatch.setenv("LK_TOPK_FUSED_MIN_ITEMS", "1")
    for name, v in kw.items():
        monkeypatch.setenv(name, str(v))


def _upload(case, gpu):
    from lkpy_amd import _device as D

    ptr, ex = C.csr(case["lists"])
    return (D.to_device_padded(case["U"], gpu), D.to_device_padded(case["Q"], gpu),
            torch.from_numpy(ptr).to(gpu), torch.from_numpy(ex).to(gpu))


def _call(case, dev, excl=True):
    from lkpy_amd import _device as D

    dU, dQ, dptr, dex = dev
    idx, sc = D.score_topk(dU, dQ, case["k"], case["n"], *((dptr, dex) if excl else ()))
    return idx, sc, D.score_topk_last_report()


def _same_bits(a, b):
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _check_oracle(oracle, case, got, rows):
    idx, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
    for b in rows:
        wi, ws = _want(oracle, case, b)
        assert np.array_equal(idx[b], wi), b
        assert np.array_equal(sc[b].view(np.uint32), ws.view(np.uint32)), b


def _check_report(rep, pred, case, designed_und, **geo):
    "the report says fused with the predicted geometry, and the redo rows are EXACTLY the predicted"
    g = pred["geometry"]
    print("report:", {k: v for k, v in rep.items() if k != "redo_rows"}, "redo", rep["redo_rows"],
          "predicted", pred["redo"], "undetermined", pred["undetermined"])
    assert rep["path"] == "fused" and not rep["all_panel"] and rep["kp"] == case["kp"]
    for key in ("batches", "parts", "part_cap", "overlap", "stride", "n_sample", "r_tau", "cmax"):
        assert rep[key] == g[key], (key, rep[key], g[key])
    for key, v in geo.items():
        assert rep[key] == v, (key, rep[key], v)
    assert rep["n_redo"] == len(rep["redo_rows"]) == len(set(rep["redo_rows"]))
    und = set(pred["undetermined"])
    assert und == set(designed_und)  # no more undetermined rows than were designed
    assert sorted(set(rep["redo_rows"]) - und) == sorted(set(pred["redo"]) - und)


def _panel_reference(monkeypatch, case, dev, excl=True):
    monkeypatch.setenv("LK_TOPK_FUSED_MIN_ITEMS", PANEL)
    idx, sc, rep = _call(case, dev, excl)
    assert rep["path"] == "panel" and rep["n_redo"] == 0 and rep["redo_rows"] == []
    monkeypatch.setenv("LK_TOPK_FUSED_MIN_ITEMS", "1")
    return idx, sc


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("k", C.WIDTHS)
def test_fused_path_every_width(gpu, oracle, monkeypatch, k, variant):
    """
    The small shape (130 x 4099, n = 10) at every width: ties between distant tiles and parts,
    all-zero items, an overflowing row, a row with fewer than n items left, lists in any order with
    repeats and entries outside the catalogue, 1 / 128 / 129 / 192 / 256 dirty sample classes, two
    rows for the second selection tier, and two knife-edge rows that keep n candidates only at
    the threshold of the right rank (r[0] = 7; r[128] = 6 with 128 classes dropped): a rank one
    off in either direction changes the redo set.  Split (4 parts of 1024) and unsplit.
    """
    case = _small(k)
    dev = _upload(case, gpu)
    _env(monkeypatch, variant)
    got = _call(case, dev)
    und = C.designed(variant[0])[1]
    _check_report(got[2], C.predict(oracle, case, stage1=variant[0]), case, und,
                  batches=1, parts=4, part_cap=1024, stride=16, n_sample=257, overlap=False,
                  cmax=variant[0] == "cmax")
    _check_oracle(oracle, case, got, range(case["B"]))
    _same_bits(got, _panel_reference(monkeypatch, case, dev))
    monkeypatch.setenv("LK_TOPK_SPLIT", "0")
    unsplit = _call(case, dev)
    _check_report(unsplit[2], C.predict(oracle, case, stage1=variant[0], split=False), case, und,
                  parts=1, part_cap=R.FUSED_CAP)
    _same_bits(got, unsplit)


@pytest.mark.parametrize("variant", [C.VARIANTS[0], C.VARIANTS[1]])
@pytest.mark.parametrize("k", [25, 100, 200])
def test_fused_non_finite_scores_slab_widths(gpu, oracle, monkeypatch, k, variant):
    "NaN column, +-inf, infinite scores inside the sample, inf * 0, the last live row of a partial tile"
    case = C.non_finite_case(k)
    dev = _upload(case, gpu)
    _env(monkeypatch, variant)
    got = _call(case, dev, excl=False)
    _check_report(got[2], C.predict(oracle, case, stage1=variant[0]), case, [], parts=4)
    _same_bits(got, _panel_reference(monkeypatch, case, dev, excl=False))
    _check_oracle(oracle, case, got, [0, 1, 4, 63, 64, 127, 128, case["B"] - 1])
    sc = got[1].cpu().numpy()
    assert not np.isnan(sc[got[0].cpu().numpy() >= 0]).any() and np.isinf(sc).any()


@pytest.mark.parametrize("variant", [C.VARIANTS[0], C.VARIANTS[1]])
@pytest.mark.parametrize("k", [64, 128, 256])
def test_fused_exact_threshold_second_tier(gpu, oracle, monkeypatch, k, variant):
    """
    LK_TOPK_TAU_EXACT=1 (r = n, every dirty class repaired: no row undetermined) with rows that
    carry more than FUSED_LCAP and at most FUSED_CAP candidates.  (On a 4099-item catalogue no
    sample divisor gets there -- the sample is at least 16 n items, a rank-n threshold passes about
    I / 16 -- so the two rows see 1500 high-scoring items OUTSIDE the sample; counts from the
    restatement.)
    """
    case = _small(k)
    dev = _upload(case, gpu)
    _env(monkeypatch, variant, LK_TOPK_TAU_EXACT=1, LK_TOPK_SAMPLE_DIV=16)
    pred = C.predict(oracle, case, stage1=variant[0], exact=True, div=16)
    assert all(R.FUSED_LCAP < pred["counts"][b] <= R.FUSED_CAP for b in C.ROWS_TIER2)
    got = _call(case, dev)
    _check_report(got[2], pred, case, [], r_tau=case["n"], parts=4)
    _same_bits(got, _panel_reference(monkeypatch, case, dev))
    _check_oracle(oracle, case, got, range(12))




@pytest.mark.parametrize("k", [128, 256])
def test_fused_in_batches_slab_widths(gpu, oracle, monkeypatch, k):
    "two fused batches (8192 + 130 rows), heavy exclusion lists on both sides of the boundary"
    case = C.expand(_small(k), 8192 + 130, C.BATCH_OVERRIDES)
    dev = _upload(case, gpu)
    _env(monkeypatch, LK_TOPK_FUSED_ROWS=8192)
    got = _call(case, dev)
    _check_report(got[2], C.predict(oracle, case, env_rows=8192), case, C.designed("cmax")[1],
                  batches=2, parts=1, overlap=False)
    _same_bits(got, _panel_reference(monkeypatch, case, dev))
    _check_oracle(oracle, case, got, [0, 1, 2, 9, 129, 130, 8190, 8191, 8192, 8193, 8321])


@pytest.mark.parametrize("k", [64, 256])
def test_fused_two_range_overlap(gpu, oracle, monkeypatch, k):
    """65 536 + 130 rows, the first size at which range A's selection runs on the side stream beside
    range B's filter: a second-tier row and a redo row on each side of the boundary."""
    case = C.expand(_small(k), 65536 + 130, C.OVERLAP_OVERRIDES)
    dev = _upload(case, gpu)
    _env(monkeypatch)
    got = _call(case, dev)
    und = C.designed("cmax")[1]
    _check_report(got[2], C.predict(oracle, case), case, und, batches=1, parts=1, overlap=True)
    monkeypatch.setenv("LK_TOPK_OVERLAP", "0")
    plain = _call(case, dev)
    _check_report(plain[2], C.predict(oracle, case, overlap=False), case, und, overlap=False)
    _same_bits(got, plain)
    _same_bits(got, _panel_reference(monkeypatch, case, dev))
    _check_oracle(oracle, case, got, [0, 1, 2, 9, 130, 65533, 65534, 65535, 65536, 65537, 65538, 65665])


@pytest.mark.parametrize("k", [64, 256])
@pytest.mark.parametrize("I,n,fused", [(C.I0, 1, True), (8192, 128, True), (8191, 128, False),
                                       (8320, 129, False)])
def test_fused_n_edges(gpu, oracle, monkeypatch, k, I, n, fused):
    "n = 1, n = FUSED_MAX_N at I = 64 n exactly and one item short of it, n = FUSED_MAX_N + 1"
    case = C.n_edge_case(k, I, n)
    dev = _upload(case, gpu)
    _env(monkeypatch)
    got = _call(case, dev)
    assert R.use_fused(case["B"], I, n, case["kp"], 1, 1) == fused
    if fused:
        _check_report(got[2], C.predict(oracle, case), case, [])
        _same_bits(got, _panel_reference(monkeypatch, case, dev))
    else:
        assert got[2]["path"] == "panel" and got[2]["batches"] == 0
    _check_oracle(oracle, case, got, range(0, case["B"], 9))


@pytest.mark.parametrize("k", [10, 300])
def test_widths_that_must_not_fuse(gpu, oracle, monkeypatch, k):
    "padded 16 (less than a staged slab) and padded 320 (beyond the fused layout): the panel path"
    case = C.small_case(k)
    dev = _upload(case, gpu)
    _env(monkeypatch)
    got = _call(case, dev)
    assert got[2]["path"] == "panel" and got[2]["kp"] == R.padded_dim(k) == case["kp"]
    assert got[2]["n_redo"] == 0 and got[2]["redo_rows"] == []
    _check_oracle(oracle, case, got, range(case["B"]))
