"""CPU: the panel loops ``SLIMScorer`` and ``AssociationScorer`` share (``knn._PanelScorer``) --
a batch cut into panels gives what one panel gives, the padding, the widths, what reaches the
scoring call, and where Association refuses a ``max_nbrs`` it has no reduction for.  The device is
the CPU here: the scoring, selection and download calls are Torch / NumPy stand-ins that record
how they were called.  With it: ``DeviceCSR.from_host`` and which scorers hand back device lists."""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

from lkpy_amd.data import ItemList, RecQuery, Vocabulary

ITEMS = Vocabulary(np.array([10, 20, 30, 40, 50]))
# hand-written 5 x 5 model: row = history / reference item, column = scored item; item 50's row
# is empty and nothing points at item 50
MODEL = np.array([[0.0, 0.5, 0.25, 0.0, 0.0],
                  [0.75, 0.0, 0.0, 0.125, 0.0],
                  [0.5, 1.5, 0.0, 4.0, 0.0],
                  [0.0, 0.0, 3.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
HISTORIES = [[10, 30], [20], [40, 10, 20], [], [50], [30, 30, 10], [20, 999, 40], [10, 20, 30, 40],
             [999]]  # [3] empty, [5] a repeat, [6] an unknown among known, [8] only an unknown
TARGETS = [[10, 20, 30, 40, 50], [50, 999, 10], [], [20, 20], [30], [40, 10], [999], [10, 50],
           [20, 30]]


def _queries():
    return [RecQuery(user_items=ItemList(np.array(h, dtype=np.int64))) for h in HISTORIES]


def _lists():
    return [ItemList(np.array(t, dtype=np.int64)) for t in TARGETS]


@pytest.fixture
def device(monkeypatch):
    "the device calls of the panel loops as CPU stand-ins; returns the record of their calls"
    from lkpy_amd import _device as D

    calls = []

    def score(kind, ptr, idx, model, reduce, rows, strike_history, nan_empty):
        calls.append((kind, rows, strike_history, nan_empty, reduce))
        assert ptr.dtype == torch.int64 and idx.dtype == torch.int32
        assert model.indptr.dtype == torch.int64
        dense = sps.csr_array((model.values.numpy(), model.indices.numpy(), model.indptr.numpy()),
                              shape=model.shape).toarray()
        lo, hi = (0, len(ptr) - 1) if rows is None else rows
        out = np.zeros((hi - lo, dense.shape[1]), np.float32)
        for r in range(lo, hi):
            own = idx[ptr[r]:ptr[r + 1]].numpy()
            known = own[own >= 0]
            for i in known:  # in history order, a repeat counted again
                out[r - lo] = np.maximum(out[r - lo], dense[i]) if reduce == "max" \
                    else out[r - lo] + dense[i]
            if reduce == "mean" and len(known):
                out[r - lo] /= np.float32(len(known))
            if strike_history:
                out[r - lo, known] = np.nan
            if nan_empty and not len(known):
                out[r - lo] = np.nan
        return torch.from_numpy(out)

    def slim_score_batch(hist_ptr, hist_items, weights, rows=None, strike_history=False,
                         nan_empty=False):
        return score("slim", hist_ptr, hist_items, weights, None, rows, strike_history, nan_empty)

    def assoc_score_batch(ref_ptr, ref_items, s, reduce, rows=None, strike_history=False,
                          nan_empty=True, out=None):
        assert out is None and reduce in ("mean", "max")
        return score("assoc", ref_ptr, ref_items, s, reduce, rows, strike_history, nan_empty)

    def argtopn(scores, n):
        calls.append(("argtopn", int(n)))
        s = scores.numpy()
        cols = s.shape[1] if n < 0 else min(int(n), s.shape[1])
        out = np.full((s.shape[0], cols), -1, np.int32)
        for r, row in enumerate(s):
            order = np.argsort(-np.where(np.isnan(row), -np.inf, row), kind="stable")
            order = order[~np.isnan(row[order])][:cols]
            out[r, :len(order)] = order
        return torch.from_numpy(out)

    def take_scores(scores, idx):
        got = torch.gather(scores, 1, idx.long().clamp(min=0))
        return torch.where(idx >= 0, got, torch.full_like(got, float("nan")))

    def record(name, fn):
        return lambda *a, **k: (calls.append((name,)), fn(*a, **k))[1]

    monkeypatch.setattr(D, "device", record("device", lambda dev=None: torch.device("cpu")))
    monkeypatch.setattr(D, "slim_score_batch", slim_score_batch)
    monkeypatch.setattr(D, "assoc_score_batch", assoc_score_batch)
    monkeypatch.setattr(D, "argtopn", argtopn)
    monkeypatch.setattr(D, "take_scores", take_scores)
    monkeypatch.setattr(D, "to_host", record("to_host", lambda t: t.numpy()))
    monkeypatch.setattr(D, "lists_to_host",
                        record("lists_to_host", lambda i, s, rows=None: (i.numpy(), s.numpy())))
    return calls


def _scorer(kind, **cfg):
    from lkpy_amd.knn import AssociationScorer, SLIMScorer

    if kind == "slim":
        sc = SLIMScorer(**cfg)
        sc.weights = sps.csr_array(MODEL)
    else:
        sc = AssociationScorer(**cfg)
        sc.assoc_scores = sps.csr_array(MODEL)
        sc.item_freqs = np.ones(5, np.int32)
    sc.items = ITEMS
    return sc


def _small_panels(monkeypatch, sc):
    "PANEL_BYTES of 4 rows of 5 float32 scores, set on the scorer's own class"
    monkeypatch.setattr(type(sc), "PANEL_BYTES", 4 * 5 * 4)
    assert sc._panel_rows() == 4


def _score_calls(calls):
    return [c for c in calls if c[0] in ("slim", "assoc")]


CASES = [("slim", {}, 3), ("slim", {}, 8), ("slim", {}, -1),
         ("assoc", {}, 3), ("assoc", {}, 8), ("assoc", {}, -1), ("assoc", {}, None),
         ("assoc", {"max_nbrs": 1}, 3)]


@pytest.mark.parametrize("kind,cfg,n", CASES)
def test_recommend_batch_in_panels(device, monkeypatch, kind, cfg, n):
    sc = _scorer(kind, **cfg)
    assert sc._panel_rows() > 9
    one_i, one_s = sc.recommend_batch(_queries(), n)
    first = _score_calls(device)
    assert [c[1:4] for c in first] == [((0, 9), True, True)]  # history struck, empty rows NaN
    assert first[0][4] == (None if kind == "slim" else "max" if cfg else "mean")
    width = 5 if n is None or n < 0 else n
    assert one_i.shape == one_s.shape == (9, width)
    assert one_i.dtype == np.int32 and one_s.dtype == np.float32
    # padding: -1 exactly where NaN, behind the listed items; candidates = items not in the history
    assert np.array_equal(one_i < 0, np.isnan(one_s))
    assert (np.diff((one_i < 0).astype(int), axis=1) >= 0).all()
    known = [sorted({ITEMS.number(i) for i in h if i != 999}) for h in HISTORIES]
    for r, own in enumerate(known):
        listed = one_i[r][one_i[r] >= 0]
        want = min(width, 5 - len(own)) if own else 0  # no known history item: nothing listed
        assert len(listed) == want and len(set(listed)) == want and not np.isin(listed, own).any()
        assert (np.diff(one_s[r, :want]) <= 0).all()
    # a row the stand-in does not decide: [10, 30] -> rows 0 + 2 of the model, items 10, 30 struck
    dense = MODEL[0] + MODEL[2]
    if kind == "assoc":
        dense = np.maximum(MODEL[0], MODEL[2]) if cfg else dense / np.float32(2)
    assert one_i[0, :3].tolist() == [3, 1, 4] and one_s[0, :3].tolist() == dense[[3, 1, 4]].tolist()

    del device[:]
    _small_panels(monkeypatch, sc)
    small_i, small_s = sc.recommend_batch(_queries(), n)
    assert [c[1] for c in _score_calls(device)] == [(0, 4), (4, 8), (8, 9)]
    assert [c[1] for c in device if c[0] == "argtopn"] == [-1 if n is None else n] * 3
    assert np.array_equal(small_i, one_i) and np.array_equal(small_s, one_s, equal_nan=True)

    del device[:]
    keep_i, _keep_s = sc.recommend_batch(_queries(), n, exclude_history=False)
    assert [c[1:4] for c in _score_calls(device)] == [((0, 4), False, True), ((4, 8), False, True),
                                                      ((8, 9), False, True)]
    assert (keep_i[7] >= 0).sum() == min(width, 5)  # the history items are candidates again


@pytest.mark.parametrize("kind,cfg", [("slim", {}), ("assoc", {}), ("assoc", {"max_nbrs": 1})])
def test_score_batch_in_panels(device, monkeypatch, kind, cfg):
    sc = _scorer(kind, **cfg)
    one = sc.score_batch(_queries(), _lists())
    # SLIM tells an empty history on the host, Association has the kernel mark it
    assert [c[1:4] for c in _score_calls(device)] == [((0, 9), False, kind == "assoc")]
    del device[:]
    _small_panels(monkeypatch, sc)
    small = sc.score_batch(_queries(), _lists())
    assert [c[1] for c in _score_calls(device)] == [(0, 4), (4, 8), (8, 9)]
    assert len(one) == len(small) == 9
    for a, b, t in zip(one, small, TARGETS):
        assert a.ids().tolist() == b.ids().tolist() == t
        sa, sb = np.asarray(a.scores(), np.float32), np.asarray(b.scores(), np.float32)
        assert sa.shape == (len(t),) and np.array_equal(sa, sb, equal_nan=True)
    got = [np.asarray(il.scores(), np.float32) for il in small]
    dense = MODEL[0] + MODEL[2]  # query 0: [10, 30]
    if kind == "assoc":
        dense = np.maximum(MODEL[0], MODEL[2]) if cfg else dense / np.float32(2)
    assert got[0].tolist() == dense.tolist()
    assert np.isnan(got[1][1]) and got[1][[0, 2]].tolist() == [0.0, 0.75]  # unknown target: NaN
    assert np.isnan(got[3]).all() and len(got[3]) == 2  # empty history
    assert got[4].tolist() == [0.0]  # a known item with an empty model row: 0.0, not NaN
    # only an unknown history item: Association has no reference item (NaN); SLIM's row is not
    # empty, so the kernel's zeros stand
    assert np.isnan(got[8]).all() if kind == "assoc" else got[8].tolist() == [0.0, 0.0]
    # one query alone (``__call__``) = its row of the batch, wherever its panel began
    for i in (0, 5, 8):
        alone = np.asarray(sc(_queries()[i], _lists()[i]).scores(), np.float32)
        assert np.array_equal(alone, got[i], equal_nan=True)


def test_association_refuses_other_limits(device):
    two = _scorer("assoc", max_nbrs=2)
    with pytest.raises(NotImplementedError, match="limited reference items"):
        two.recommend_batch(_queries(), 3)
    assert device == []  # refused before anything is uploaded or scored
    with pytest.raises(NotImplementedError):
        two.dense_scores_batch(_queries())
    assert device == []
    # score_batch: the reference raises once it has reference items, not before
    no_refs = [_queries()[3], _queries()[8]]
    got = two.score_batch(no_refs, [_lists()[0]] * 2)
    assert all(np.isnan(np.asarray(il.scores())).all() and len(il) == 5 for il in got)
    with pytest.raises(NotImplementedError):
        two.score_batch(no_refs + [_queries()[6]], [_lists()[0]] * 3)


def test_from_host_uploads_a_model_matrix():
    from lkpy_amd import _device as D

    mat = sps.csr_array(MODEL)
    assert mat.indptr.dtype == np.int32  # SciPy's offsets; the batch scoring calls want int64
    indptr, indices, data = mat.indptr.copy(), mat.indices.copy(), mat.data.copy()
    views = [a.view() for a in (indptr, indices, data)]
    for v in views:
        v.flags.writeable = False  # what a zero-copy view of an Arrow buffer looks like
    cpu = torch.device("cpu")
    csr = D.DeviceCSR.from_host(*views, (np.int64(5), np.int64(5)), cpu)
    assert csr.indptr.dtype == torch.int64 and csr.indices.dtype == torch.int32
    assert csr.values.dtype == torch.float32 and csr.shape == (5, 5) and csr.nnz == mat.nnz
    assert all(type(x) is int for x in csr.shape)
    assert csr.indptr.tolist() == mat.indptr.tolist()
    assert csr.indices.tolist() == mat.indices.tolist()
    assert csr.values.tolist() == mat.data.tolist()
    for v, a, b in zip(views, (indptr, indices, data), (mat.indptr, mat.indices, mat.data)):
        assert not v.flags.writeable and np.array_equal(a, b) and a.dtype == b.dtype
    # structure only; unsorted rows stay as they are; float64 values are cast
    rows = D.DeviceCSR.from_host(np.array([0, 2, 3]), np.array([4, 1, 2], np.int64), None, (2, 5),
                                 cpu)
    assert rows.values is None and rows.indptr.dtype == torch.int64
    assert rows.indices.tolist() == [4, 1, 2] and rows.indices.dtype == torch.int32
    wide = D.DeviceCSR.from_host(mat.indptr, mat.indices, mat.data.astype(np.float64), (5, 5), cpu)
    assert wide.values.dtype == torch.float32 and wide.values.tolist() == mat.data.tolist()


def test_which_scorers_return_device_lists():
    "``batch.recommend`` reads the attribute; it says what the signature of recommend_batch says"
    import inspect

    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.flexmf import FlexMFExplicitScorer, FlexMFImplicitScorer
    from lkpy_amd.knn import AssociationScorer, ItemKNNScorer, SLIMScorer

    for cls, want in ((ImplicitMFScorer, True), (FlexMFImplicitScorer, True),
                      (FlexMFExplicitScorer, True), (ItemKNNScorer, False), (SLIMScorer, False),
                      (AssociationScorer, False)):
        assert getattr(cls(), "returns_device_lists", False) is want, cls
        assert ("device_output" in inspect.signature(cls.recommend_batch).parameters) is want
