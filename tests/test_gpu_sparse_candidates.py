"""GPU parity, kernel level: ``lk_sparse_score_candidates`` (csrc/sparse_candidates.hip) against
``tests/sparse_candidates_restatement`` AND against the panel path it replaces --
``lk_slim_score_batch`` / ``lk_assoc_score_batch`` followed by ``lk_panel_take_ragged`` -- on
hand-made inputs at the smallest shapes that can go wrong.  The chain has a fixed order, so every
comparison is bit equality."""
import functools

import numpy as np
import pytest
import torch

import sparse_candidates_restatement as R

pytestmark = pytest.mark.gpu

# target list lengths: empty first / in the middle / last, 1, the wave seam (63, 64, 65: query
# boundaries inside a wave from the second list on), short ones, one of several waves
LAYOUT = [0, 1, 63, 64, 65, 7, 7, 0, 130, 2, 0]
# history rows (item numbers; whatever is outside [0, n_items) is an unknown item)
HISTORIES = [
    [],                                  # 0: no entries at all
    [-1, -1],                            # 1: only unknown items
    [3, -1, 4],                          # 2: an unknown item in the middle
    [4, 4, 2],                           # 3: the same item twice
    [0, 1],                              # 4: item 0's model row is empty
    [10, 11, 12],                        # 5: column 5 holds 1e8, 1, -1e8 in these rows ...
    [10, 12, 11],                        # 6: ... and in this order the sum differs
    [3, 4, 1, 2, 20, 21, 22, 23, 3, 5],  # 7: long rows, a repeat; m exceeds the rows with a column
    [100000],                            # 8: only an item past every model
    [0],                                 # 9: a known item whose row is empty: m = 1, nothing added
    [5, 6, 7, 8],                        # 10: the 300-entry row where the model has it
]
# with row numbers: every query reads another row than its own; -1 and 11 are outside the CSR
ROWS = [3, 0, 7, 5, 6, 2, 4, 1, 7, 11, -1]
ROW_LENS = {0: 0, 1: 1, 2: 2, 3: 64, 4: 65, 5: 300}  # the other rows: 0 .. 20 entries


def _ptr(lens):
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr


@functools.lru_cache(maxsize=None)
def _case(n_items):
    "(history ptr, items, model ptr, idx, val, target ptr, items) for one model size"
    rng = np.random.default_rng(900 + n_items)
    rows_idx, rows_val = [], []
    for r in range(n_items):
        want = min(ROW_LENS.get(r, int(rng.integers(0, 21))), n_items)
        if n_items == 1:
            want = 1  # (the one cell there is)
        forced = [c for c in ((5, 7) if r in (3, 4, 5, 10, 11, 12) else ()) if c < n_items]
        want = max(want, len(forced))
        rest = np.setdiff1d(np.arange(n_items), forced)
        cols = np.sort(np.concatenate([forced, rng.choice(rest, want - len(forced), replace=False)
                                       ]).astype(np.int32))
        vals = rng.standard_normal(len(cols)).astype(np.float32)
        vals[rng.random(len(cols)) < 0.05] = -0.0
        vals[cols == 7] = -np.abs(vals[cols == 7]) - np.float32(0.5)  # an all-negative column
        if r in (10, 11, 12):
            vals[cols == 5] = {10: 1.0e8, 11: 1.0, 12: -1.0e8}[r]
        rows_idx.append(cols)
        rows_val.append(vals)
    m_ptr = _ptr([len(c) for c in rows_idx])
    m_idx = np.concatenate(rows_idx).astype(np.int32) if rows_idx else np.zeros(0, np.int32)
    m_val = np.concatenate(rows_val).astype(np.float32) if rows_val else np.zeros(0, np.float32)
    h_ptr = _ptr([len(h) for h in HISTORIES])
    h_idx = np.array([i for h in HISTORIES for i in h], np.int32)
    t_ptr = _ptr(LAYOUT)
    tgt = rng.integers(0, n_items, int(t_ptr[-1])).astype(np.int32)
    first, last = (rows_idx[3][0], rows_idx[3][-1]) if n_items > 3 else (0, 0)
    for q, n in enumerate(LAYOUT):
        lo = int(t_ptr[q])
        if n >= 5:  # the columns above; an edge of row 3; the same target twice
            tgt[lo:lo + 5] = [5, 7, first, last, 5]
        if n >= 7:
            tgt[lo + 5:lo + 7] = [-1, n_items]
    return h_ptr, h_idx, m_ptr, m_idx, m_val, t_ptr, tgt


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(R.bits(got)[~nan], R.bits(want)[~nan])


def _operands(D, gpu, n_items):
    h_ptr, h_idx, m_ptr, m_idx, m_val, _t_ptr, _tgt = _case(n_items)
    hist = D.DeviceCSR.from_arrays(h_ptr, h_idx, None, (len(HISTORIES), n_items), gpu)
    model = D.DeviceCSR.from_host(m_ptr, m_idx, m_val, (n_items, n_items), gpu)
    return hist, model


def _panel_path(D, gpu, n_items, rows, reduce, t_ptr, tgt):
    "the composition the kernel replaces: the histories in query order -> panel -> ragged take"
    h_ptr, h_idx, *_ = _case(n_items)
    _hist, model = _operands(D, gpu, n_items)
    n_q = len(t_ptr) - 1
    pick = range(n_q) if rows is None else rows
    lists = [h_idx[h_ptr[r]:h_ptr[r + 1]] if 0 <= r < len(HISTORIES) else h_idx[:0] for r in pick]
    q_ptr = _dev(_ptr([len(x) for x in lists]), gpu)
    q_idx = _dev(np.concatenate(lists).astype(np.int32), gpu)
    if reduce == "sum":
        panel = D.slim_score_batch(q_ptr, q_idx, model, nan_empty=True)
    else:
        panel = D.assoc_score_batch(q_ptr, q_idx, model, reduce, nan_empty=True)
    return _host(D.panel_take_ragged(panel, n_items, _dev(t_ptr, gpu), _dev(tgt, gpu), t_ptr))


@pytest.mark.parametrize("with_rows", [False, True], ids=["by-position", "by-row-number"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("n_items", [1, 70, 330])
def test_kernel_is_the_restatement_and_the_panel_cell(gpu, n_items, reduce, with_rows):
    from lkpy_amd import _device as D

    h_ptr, h_idx, m_ptr, m_idx, m_val, t_ptr, tgt = _case(n_items)
    lens = set(np.diff(m_ptr).tolist())
    assert {0, 1} & lens and (n_items < 70 or {0, 1, 2, 64, 65} <= lens)
    assert n_items < 330 or 300 in lens
    assert (tgt == -1).any() and (tgt == n_items).any()
    rows = ROWS if with_rows else None
    hist, model = _operands(D, gpu, n_items)
    got = _host(D.sparse_score_candidates(
        hist, model, reduce, _dev(t_ptr, gpu), _dev(tgt, gpu), t_ptr,
        rows=_dev(np.array(ROWS, np.int32), gpu) if with_rows else None))
    want = R.sparse_score_candidates_ref(h_ptr, h_idx, rows, m_ptr, m_idx, m_val, n_items,
                                         t_ptr, tgt, reduce)
    assert _same_bits(got, want)
    assert _same_bits(got, _panel_path(D, gpu, n_items, rows, reduce, t_ptr, tgt))

    # what the inputs were made to show
    seg = lambda q: got[int(t_ptr[q]):int(t_ptr[q + 1])]  # noqa: E731
    assert np.isnan(got[(tgt < 0) | (tgt >= n_items)]).all()
    if with_rows:
        assert np.isnan(seg(1)).all()  # history row 0: no entries at all
        assert np.isnan(seg(9)).all()  # a row number outside the CSR
    else:  # history row 1, unknown items alone (the one target is a valid column)
        assert seg(1)[0] == 0 if reduce == "sum" else np.isnan(seg(1)[0])
    if n_items >= 70:
        # column 5 (the first target of a list) over the histories 10, 11, 12 and 10, 12, 11
        q_a, q_b = (3, 4) if with_rows else (5, 6)
        assert (seg(q_a)[0], seg(q_b)[0]) == {
            "sum": (0.0, 1.0), "mean": (0.0, np.float32(1.0 / 3.0)), "max": (1.0e8, 1.0e8)}[reduce]
        # column 7 (the second target) is negative wherever it is held: history 3, 4, ... with
        # row numbers, history 4, 4, 2 without
        c7 = seg(2 if with_rows else 3)[1]
        assert (c7 == 0 and not np.signbit(c7)) if reduce == "max" else c7 < 0
    if n_items == 70:  # (the comparison is not one of NaNs and zeros)
        assert np.isfinite(got).sum() > 150 and (got[np.isfinite(got)] != 0).sum() > 50


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_a_result_depends_on_its_own_segment_alone(gpu, reduce):
    from lkpy_amd import _device as D

    n_items = 70
    _h_ptr, _h_idx, _m_ptr, _m_idx, _m_val, t_ptr, tgt = _case(n_items)
    hist, model = _operands(D, gpu, n_items)
    rows = np.array(ROWS, np.int32)
    whole = _host(D.sparse_score_candidates(hist, model, reduce, _dev(t_ptr, gpu),
                                            _dev(tgt, gpu), t_ptr, rows=_dev(rows, gpu)))
    for q in (2, 8):
        lo, hi = int(t_ptr[q]), int(t_ptr[q + 1])
        one = np.array([0, hi - lo], np.int64)
        alone = _host(D.sparse_score_candidates(hist, model, reduce, _dev(one, gpu),
                                                _dev(tgt[lo:hi], gpu), one,
                                                rows=_dev(rows[q:q + 1], gpu)))
        assert _same_bits(alone, whole[lo:hi])


def test_no_targets_no_launch_and_bad_arguments(gpu):
    from lkpy_amd import _device as D

    hist, model = _operands(D, gpu, 70)
    empty = np.zeros(len(HISTORIES) + 1, np.int64)
    none = _dev(np.zeros(0, np.int32), gpu)
    for ptr in (empty, np.zeros(1, np.int64)):
        out = D.sparse_score_candidates(hist, model, "sum", _dev(ptr, gpu), none, ptr)
        assert out.shape == (0,) and out.dtype == torch.float32
    with pytest.raises(ValueError, match="unknown reduction"):
        D.sparse_score_candidates(hist, model, "median", _dev(empty, gpu), none, empty)
    with pytest.raises(ValueError, match="tgt_ptr"):
        D.sparse_score_candidates(hist, model, "sum", _dev(empty, gpu),
                                  _dev(np.zeros(3, np.int32), gpu), empty)
