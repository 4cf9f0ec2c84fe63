"""GPU parity: the full descending sort behind top-N (csrc/topn_sort.hip on csrc/radix_sort.h, 64-bit
keys ``(row << 32) | ~score-key`` with ``<uint64, uint32>`` pairs) -- ``lk_argtopn`` and
``lk_score_topk`` with ``n < 0`` or ``n > 4096`` -- at the edges of the sort.

The order is defined: score descending, then lower index; NaN dropped; -0.0 ranks with +0.0; rows
padded with -1 and NaN.  ``oracle.argsort_descending`` (NumPy's stable sort of the negated float32
scores) gives exactly that order, so every comparison is equality: indices entry for entry, scores
bit for bit.  Each test first asserts, on its own inputs, that the edges it claims are present."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 4096  # keys per workgroup of the sort (radix_sort.h)
TOPN_MAX = 4096  # longest list of the selection kernel (topk.hip)
SENTINEL = -0x5A5A5A5B  # no index and not -1

NAN_BITS = np.array([0x7FC00000, 0xFFC00001, 0x7FA00000, 0xFF800001, 0x7FFFFFFF], np.uint32)
CLASSES = ["normal", "tenths", "constant", "zeros", "infs", "denormals", "nan bits", "all nan",
           "single valid"]
TIED = ("tenths", "constant", "zeros", "denormals")


def _row(kind, n, rng):
    "one row of a data class, as float32 (NaNs are written as bit patterns)"
    x = rng.standard_normal(n).astype(np.float32)
    u = x.view(np.uint32)
    if kind == "tenths":  # heavy ties, the heaviest at both ends of the ranking
        x[:] = np.round(np.clip(x, -1.5, 1.5), 1)
    elif kind == "constant":
        x[:] = 1.5
    elif kind == "zeros":  # alternating -0.0 / +0.0
        u[:] = 0
        u[::2] = 0x80000000
    elif kind == "infs":
        x[rng.random(n) < 0.05] = np.inf
        x[rng.random(n) < 0.05] = -np.inf
        x[0], x[-1] = np.inf, -np.inf
    elif kind == "denormals":  # both signs; half of the row shares the 39 largest magnitudes, so
        # that equal scores open and close the ranking
        mant = rng.integers(1, 1 << 22, n).astype(np.uint32)
        few = rng.random(n) < 0.5
        mant[few] = (1 << 23) - rng.integers(1, 40, int(few.sum()))
        u[:] = mant | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    elif kind == "nan bits":
        at = np.flatnonzero(rng.random(n) < 0.2)
        u[at] = NAN_BITS[np.arange(len(at)) % len(NAN_BITS)]
        u[n // 2] = NAN_BITS[1]
    elif kind == "all nan":
        u[:] = NAN_BITS[np.arange(n) % len(NAN_BITS)]
    elif kind == "single valid":
        keep = u[n // 3]
        u[:] = NAN_BITS[np.arange(n) % len(NAN_BITS)]
        u[n // 3] = keep
    else:
        assert kind == "normal"
    return x


def _matrices(rng, rows, row_len):
    """Score matrices [rows x row_len] whose rows run through every data class: one matrix where it
    has rows enough, otherwise as many as it takes."""
    out = []
    for first in range(0, len(CLASSES), rows):
        kinds = [CLASSES[(first + r) % len(CLASSES)] for r in range(rows)]
        out.append((np.stack([_row(k, row_len, rng) for k in kinds]), kinds))
        if rows >= len(CLASSES):
            break
    assert {k for _s, kinds in out for k in kinds} == set(CLASSES)
    return out


def _classes_present(s, kinds):
    "what the rows of a matrix are said to hold, they hold"
    u = s.view(np.uint32)
    n = s.shape[1]
    for r, kind in enumerate(kinds):
        nan = np.isnan(s[r])
        if kind == "tenths" and n > 100:
            assert len(np.unique(s[r])) < n // 4
        if kind == "constant":
            assert len(np.unique(u[r])) == 1
        if kind == "zeros":
            assert not s[r].any() and u[r, 0] == 0x80000000 and (n < 2 or u[r, 1] == 0)
        if kind == "infs":
            assert np.isneginf(s[r, -1]) and (np.isposinf(s[r, 0]) or n == 1)
        if kind == "denormals":
            mag = u[r] & 0x7FFFFFFF
            assert (mag > 0).all() and (mag < 0x00800000).all()
            assert n < 10 or len(np.unique(u[r] >> 31)) == 2
        if kind == "nan bits":
            assert u[r, n // 2] == 0xFFC00001 and (n < 100 or (u[r] == 0x7FA00000).any())
            assert n < 100 or not nan.all()
        if kind == "all nan":
            assert nan.all() and (n < 5 or len(np.unique(u[r])) == len(NAN_BITS))
        if kind == "single valid":
            assert (~nan).sum() == 1
        if kind in ("normal", "tenths", "constant", "zeros", "infs", "denormals"):
            assert not nan.any()


def _row_bits(rows):
    b = 0
    while (1 << b) < rows:
        b += 1
    return b


def _sort_shape(rows, row_len):
    "tiles, key bits, passes and the width of the last digit of topn_sort's sort of one batch"
    assert rows * row_len <= 1 << 28  # one batch (sort_batch_rows)
    bits = 32 + _row_bits(rows)
    passes = (bits + 7) // 8
    return (rows * row_len + TILE - 1) // TILE, bits, passes, bits - 8 * (passes - 1)


def _want_full(oracle, s):
    want = np.full(s.shape, -1, np.int32)
    for r in range(s.shape[0]):
        w = oracle.argsort_descending(s[r])
        want[r, :len(w)] = w
    return want


# (rows, row_len) -> (tiles, key bits, passes, bits of the last digit)
ARGTOPN_SHAPES = {
    (1, 4097): (2, 32, 4, 8),      # an even pass count: the first pass goes to the tmp pair
    (1, 1): (1, 32, 4, 8),
    (300, 5): (1, 41, 6, 1),       # hundreds of rows inside one tile
    (3, 5000): (4, 34, 5, 2),      # row boundaries inside tiles
    (257, 4100): (258, 41, 6, 1),  # more than 256 tiles: the scan's second trip and its carry
}


@pytest.mark.parametrize("rows,row_len", list(ARGTOPN_SHAPES))
def test_argtopn_sort_path_against_the_reference(gpu, oracle, rng, rows, row_len):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    assert _sort_shape(rows, row_len) == ARGTOPN_SHAPES[(rows, row_len)]
    if (rows, row_len) == (1, 4097):
        assert row_len - TILE == 1  # the second tile holds one key
    if rows == 257:
        assert _sort_shape(rows, row_len)[0] > 256
    lib = _native.require_gpu()
    seen_tie_at_cut = set()
    for m, (s, kinds) in enumerate(_matrices(rng, rows, row_len)):
        _classes_present(s, kinds)
        d = torch.from_numpy(s).to(gpu)
        assert np.array_equal(d.cpu().numpy().view(np.uint32), s.view(np.uint32))  # NaN payloads kept
        want = _want_full(oracle, s)
        full = D.argtopn(d, -1).cpu().numpy()
        assert full.shape == (rows, row_len)
        for r in range(rows):
            assert np.array_equal(full[r], want[r]), (m, r, kinds[r])

        if m == 0:  # the ABI itself, over an output full of a sentinel
            out = torch.full((rows, row_len), SENTINEL, dtype=torch.int32, device=gpu)
            wb = lib.lk_argtopn_workspace_bytes(rows, row_len, -1)
            assert wb > 0
            ws = torch.empty(wb, dtype=torch.uint8, device=gpu)
            _native.check(lib.lk_argtopn(D._ptr(d), rows, row_len, -1, D._ptr(ws), D._ptr(out),
                                         D._stream()), "lk_argtopn")
            out = out.cpu().numpy()
            assert not (out == SENTINEL).any() and np.array_equal(out, want)

        if row_len > TOPN_MAX + 1:
            # longer lists than the selection kernel holds are prefixes of the full ranking ...
            for n in (TOPN_MAX + 1, row_len - 1):
                got = D.argtopn(d, n).cpu().numpy()
                assert got.shape == (rows, n) and np.array_equal(got, full[:, :n]), n
            # ... and the selection kernel's longest list is a prefix of the sort's: "the two
            # paths agree on every prefix", on rows where equal scores straddle the cut
            sel = D.argtopn(d, TOPN_MAX).cpu().numpy()
            for r in range(rows):
                a, b = full[r, TOPN_MAX - 1], full[r, TOPN_MAX]
                if kinds[r] in TIED:
                    assert a >= 0 and b >= 0 and s[r, a] == s[r, b], (r, kinds[r])
                    seen_tie_at_cut.add(kinds[r])
                assert np.array_equal(sel[r], full[r, :TOPN_MAX]), (m, r, kinds[r])
    if row_len > TOPN_MAX + 1:
        assert seen_tie_at_cut == set(TIED)


def test_argtopn_short_rows_take_the_sort_only_when_asked(gpu, oracle, rng):
    "300 x 5 and 1 x 1 reach the sort through n = -1 alone: the same lists as the selection kernel"
    from lkpy_amd import _device as D

    for rows, row_len in ((1, 1), (300, 5)):
        for s, kinds in _matrices(rng, rows, row_len):
            d = torch.from_numpy(s).to(gpu)
            full = D.argtopn(d, -1).cpu().numpy()
            sel = D.argtopn(d, row_len).cpu().numpy()
            assert np.array_equal(full, _want_full(oracle, s)) and np.array_equal(sel, full)


# ---- lk_score_topk, full path, two panels ---------------------------------------------------------

PANEL = 2048  # user rows per score panel (topk.hip: SCORE_BATCH_DEFAULT)


@pytest.fixture(scope="module")
def topk_case():
    "operands, exclusion lists and the rows that are checked: built once, never changed"
    rng = np.random.default_rng(17)
    B, n_items, k = PANEL + 70, 4200, 8
    U = rng.standard_normal((B, k)).astype(np.float32)
    Q = rng.standard_normal((n_items, k)).astype(np.float32)
    zero = rng.permutation(n_items)[: n_items // 20]
    Q[zero] = 0.0  # 5 % of the items score zero for everybody
    Q[3000:3100] = Q[100:200]  # exact ties for every user
    lists = [rng.integers(0, n_items, int(rng.integers(0, 40))) for _ in range(B)]
    sparse = (5, PANEL + 9)  # one row in each panel keeps three items
    lists[0] = np.empty(0, np.int64)
    for b in sparse:
        lists[b] = rng.permutation(n_items)[3:]
    # the first row of the second panel: a long list with repeats and entries that name no item
    lists[PANEL] = np.concatenate([rng.integers(0, n_items, 3000), [-1, n_items, n_items + 7]])
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    items = np.concatenate(lists).astype(np.int32)
    check = sorted({0, 1, PANEL - 1, PANEL, PANEL + 1, B - 1, *sparse,
                    *rng.integers(0, B, 4).tolist()})
    for a in (U, Q, ptr, items):
        a.setflags(write=False)
    return dict(B=B, n_items=n_items, k=k, U=U, Q=Q, zero=zero, ptr=ptr, items=items,
                sparse=sparse, check=check)


def _topk_reference(oracle, c, b):
    s = oracle.score_dense(c["Q"], c["U"][b])
    ex = c["items"][c["ptr"][b]:c["ptr"][b + 1]]
    s[ex[(ex >= 0) & (ex < c["n_items"])]] = np.nan
    return s, oracle.argsort_descending(s)


def test_score_topk_full_path_over_two_panels(gpu, oracle, topk_case):
    from lkpy_amd import _device as D

    c = topk_case
    B, n_items, k = c["B"], c["n_items"], c["k"]
    # the edges: two panels (the second 70 rows: 39 key bits, 5 passes; the first 43 bits, 6),
    # a padded panel stride, output rows at ub * out_cols, lists that name almost every item
    assert "LK_SCORE_BATCH" not in os.environ and PANEL < B < 2 * PANEL
    assert _sort_shape(PANEL, n_items) == (2100, 43, 6, 3)
    assert _sort_shape(B - PANEL, n_items) == (72, 39, 5, 7)
    ld_s = (n_items + 63) // 64 * 64
    assert ld_s == 4224 != n_items and n_items > TOPN_MAX
    assert c["ptr"][1] == 0 and c["ptr"][PANEL + 1] - c["ptr"][PANEL] > 3000
    assert all(b // PANEL == p for p, b in enumerate(c["sparse"]))
    assert {0, 1, PANEL - 1, PANEL, PANEL + 1, B - 1, *c["sparse"]} <= set(c["check"])
    ref = {b: _topk_reference(oracle, c, b) for b in c["check"]}
    for b, (s, want) in ref.items():
        valid = len(want)
        assert valid == (3 if b in c["sparse"] else n_items if b == 0 else valid)
        assert not (s.view(np.uint32) == 0x80000000).any()  # (the key image would lose a -0.0)
        if b not in c["sparse"] and b != PANEL:
            # of two items with the same score bits the lower index ranks first
            su = s.view(np.uint32)
            live = ~np.isnan(s[100:200]) & ~np.isnan(s[3000:3100])
            assert live.sum() > 50 and np.array_equal(su[100:200][live], su[3000:3100][live])
            rank = np.empty(n_items, np.int64)
            rank[want] = np.arange(valid)
            assert (rank[3000:3100][live] > rank[100:200][live]).all()
            assert (s[c["zero"]] == 0).sum() > 100  # and a block of equal zero scores

    dU, dQ = D.to_device_padded(c["U"], gpu), D.to_device_padded(c["Q"], gpu)
    dptr = torch.from_numpy(c["ptr"].copy()).to(gpu)
    dex = torch.from_numpy(c["items"].copy()).to(gpu)
    res = {}
    for n in (-1, 4100, 4300):
        cols = n_items if n < 0 else n
        assert n < 0 or n > TOPN_MAX
        idx, sc = D.score_topk(dU, dQ, k, n, dptr, dex)
        assert tuple(idx.shape) == (B, cols) and tuple(sc.shape) == (B, cols)
        res[n] = (idx, sc)
        rows = torch.tensor(c["check"], device=gpu)
        gi, gs = idx[rows].cpu().numpy(), sc[rows].cpu().numpy()
        for j, b in enumerate(c["check"]):
            s, want = ref[b]
            m = min(len(want), cols)
            assert np.array_equal(gi[j, :m], want[:m]), (n, b)
            assert np.array_equal(gs[j, :m].view(np.uint32), s[want[:m]].view(np.uint32)), (n, b)
            assert (gi[j, m:] == -1).all() and np.isnan(gs[j, m:]).all(), (n, b)
    assert 4300 > n_items  # more columns than items: every row ends in padding
    assert bool((res[4300][0][:, n_items:] == -1).all())
    assert bool(torch.isnan(res[4300][1][:, n_items:]).all())
    # every row of both panels: the shorter list is the longer one's prefix, bits included
    for n, wider in ((4100, -1), (-1, 4300)):
        cols = n_items if n < 0 else n
        assert torch.equal(res[n][0], res[wider][0][:, :cols])
        assert torch.equal(res[n][1].view(torch.int32), res[wider][1][:, :cols].view(torch.int32))
    # no row without a list: only excluded or absent entries are -1
    counts = (res[-1][0] >= 0).sum(dim=1).cpu().numpy()
    assert counts[0] == n_items and all(counts[b] == 3 for b in c["sparse"])
    assert counts.min() == 3 and (counts[list(c["check"])] == [len(ref[b][1]) for b in c["check"]]).all()
