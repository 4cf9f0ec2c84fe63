"""
Association rules on the device (csrc/assoc.hip, ``lkpy_amd.knn.AssociationScorer``) against the
NumPy / SciPy restatement of ``tests/assoc_restatement.py``.

Bar: everything is BIT-identical to the restatement -- the learned matrix (NumPy's in-place
float64 divisions and float32 multiply), the scores (``np.mean`` adds a cell's values in
reference-item order: the synthetic kernel input has values over nine decades, so a reordered sum
shows, ``tests/test_assoc_host.py`` asserts that about this very input) and the listed scores.
Recommendation lists may differ from the restatement's only among items of bit-equal score.
"""
import pickle
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import assoc_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
CONFIGS = [("probability", 0.0), ("lift", 0.0), ("lift", 20.0), ("lift", 10.5)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    "NaN where the restatement has NaN, the same bits everywhere else"
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN cells differ"
    ok = ~np.isnan(want)
    bad = np.flatnonzero(_bits(got[ok]) != _bits(want[ok]))
    assert len(bad) == 0, f"{what}: {len(bad)} cells differ in bits, first at {bad[:5]}"


def _upload(s, gpu):
    import torch

    from lkpy_amd import _device as D

    return D.DeviceCSR(torch.from_numpy(s.indptr.astype(np.int64)).to(gpu),
                       torch.from_numpy(s.indices.astype(np.int32)).to(gpu),
                       torch.from_numpy(s.data.astype(np.float32)).to(gpu),
                       (int(s.shape[0]), int(s.shape[1])), None)


def _pack(queries, gpu):
    import torch

    ptr = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(q) for q in queries], out=ptr[1:])
    idx = np.concatenate(queries).astype(np.int32) if len(queries) else np.zeros(0, np.int32)
    return torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)


SIZES = {"1": lambda w: 1, "63": lambda w: 63, "64": lambda w: 64, "65": lambda w: 65,
         "W-1": lambda w: w - 1, "W": lambda w: w, "W+1": lambda w: w + 1,
         "2W+3": lambda w: 2 * w + 3}


@pytest.mark.parametrize("size", list(SIZES))
def test_score_kernel_equals_restatement_bit_for_bit(gpu, size):
    import torch

    from lkpy_amd import _device as D

    n = SIZES[size](D.assoc_window())
    s, queries = R.kernel_case(n)
    lens = np.diff(s.indptr)
    assert lens[0] == n and (n < 2 or lens[1] == 0) and (n < 3 or lens[2] == 1)
    assert n < 1000 or lens[3] > 256  # longer than one workgroup stride
    ds = _upload(s, gpu)
    ptr, idx = _pack(queries, gpu)
    p1, i1 = _pack([queries[R.PROBE]], gpu)
    pad = 5
    for reduce in ("mean", "max"):
        base = [R.reduce_rows(s, q, 1 if reduce == "max" else None) for q in queries]
        assert base[0] is None and base[1] is None and base[2] is not None
        for mark in range(4):
            out = torch.full((len(queries), n + pad), 7.25, dtype=torch.float32, device=gpu)
            got = D.assoc_score_batch(ptr, idx, ds, reduce, strike_history=bool(mark & 1),
                                      nan_empty=bool(mark & 2), out=out).cpu().numpy()
            assert (got[:, n:] == 7.25).all(), "padding beyond n_items was written"
            for qi, q in enumerate(queries):
                _assert_same(got[qi, :n], R.mark_row(base[qi], q, n, mark),
                             f"n={n} {reduce} mark={mark} query {qi}")
            # the probe query alone: the bits it has as row 7 of the batch of 9
            alone = D.assoc_score_batch(p1, i1, ds, reduce, strike_history=bool(mark & 1),
                                        nan_empty=bool(mark & 2)).cpu().numpy()
            assert alone.shape == (1, n)
            assert np.array_equal(_bits(alone[0]), _bits(got[R.PROBE, :n]))
            # a sub-range of the batch: rows (4, 8)
            part = D.assoc_score_batch(ptr, idx, ds, reduce, rows=(4, 8),
                                       strike_history=bool(mark & 1),
                                       nan_empty=bool(mark & 2)).cpu().numpy()
            assert np.array_equal(_bits(part), _bits(got[4:8, :n]))


def test_score_kernel_rejects_bad_arguments(gpu):
    import torch

    from lkpy_amd import _device as D

    s, queries = R.kernel_case(65)
    ds = _upload(s, gpu)
    ptr, idx = _pack(queries, gpu)
    with pytest.raises(ValueError):
        D.assoc_score_batch(ptr, idx, ds, "median")
    narrow = torch.zeros((len(queries), 64), dtype=torch.float32, device=gpu)
    with pytest.raises(AssertionError):
        D.assoc_score_batch(ptr, idx, ds, "mean", out=narrow)
    with pytest.raises(ValueError):
        D.assoc_scale(ds, torch.ones(65, dtype=torch.int32, device=gpu), 10, "cosine", 0.0)


@pytest.mark.parametrize("n_groups", [671, 2 ** 24 + 1])
def test_scale_kernel_equals_numpy_in_place(gpu, n_groups):
    import torch

    from lkpy_amd import _device as D

    rng = np.random.default_rng(77)
    n = 700
    mat = sps.random_array((n, n), density=0.05, rng=rng, format="csr")
    mat.sort_indices()
    counts = rng.integers(1, 70001, mat.nnz).astype(np.float32)
    counts[:4] = [1, 70000, 2, 69999]
    item_counts = rng.integers(1, 70001, n).astype(np.int32)
    item_counts[:4] = [1, 70000, 3, 7]
    rows = np.repeat(np.arange(n), np.diff(mat.indptr))
    d_counts = torch.from_numpy(item_counts).to(gpu)
    for method in ("probability", "lift"):
        for damping in (0.0, 20.0, 10.5, 0.1):
            want = R.scale(counts, rows, mat.indices, item_counts, n_groups, method, damping)
            csr = _upload(sps.csr_array((counts, mat.indices, mat.indptr), shape=(n, n)), gpu)
            got = D.assoc_scale(csr, d_counts, n_groups, method, damping)
            assert got is csr
            assert np.array_equal(_bits(got.values.cpu().numpy()), _bits(want)), \
                (method, damping, n_groups)
            assert np.array_equal(got.indices.cpu().numpy(), mat.indices)


# -- ml-latest-small end to end ------------------------------------------------------------------

@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def ml_counts(ml_ds):
    "the restatement's co-occurrence counts, formed once"
    cooc, item_counts, n_groups = R.cooc_counts(ml_ds.interaction_matrix())
    assert n_groups == 671 and cooc.shape == (9125, 9125) and cooc.nnz > 20_000_000
    return cooc, item_counts, n_groups


@pytest.fixture(scope="module")
def ml_lift20(gpu, ml_ds, ml_counts):
    "(scorer trained with the biased-lift.toml settings, the restatement's matrix)"
    from lkpy_amd.knn import AssociationScorer

    scorer = AssociationScorer(method="lift", damping=20)
    scorer.train(ml_ds)
    return scorer, R.train(*ml_counts, "lift", 20.0)


@pytest.mark.parametrize("method,damping", CONFIGS)
def test_training_equals_restatement_bit_for_bit(gpu, ml_ds, ml_counts, method, damping):
    from lkpy_amd.knn import AssociationScorer

    scorer = AssociationScorer(method=method, damping=damping)
    assert not scorer.is_trained()
    scorer.train(ml_ds)
    assert scorer.is_trained() and scorer.items is ml_ds.items
    got, want = scorer.assoc_scores, R.train(*ml_counts, method, damping)
    assert isinstance(got, sps.csr_array) and got.dtype == np.float32 and got.shape == want.shape
    assert scorer.item_freqs.dtype == np.int32
    assert np.array_equal(scorer.item_freqs, ml_counts[1])
    assert np.array_equal(got.indptr, want.indptr), "row lengths differ"
    assert np.array_equal(got.indices, want.indices), "indices differ"
    assert np.array_equal(_bits(got.data), _bits(want.data)), "value bits differ"
    assert (got.diagonal() == 0).all() and (np.diff(got.indptr)[ml_counts[1] == 0] == 0).all()


def test_component_scores(gpu, ml_ds, ml_lift20):
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.knn import AssociationScorer

    scorer, s = ml_lift20
    ids = ml_ds.items.ids()
    n_items = len(ids)
    all_items = ItemList(item_ids=np.concatenate([ids, [10 ** 9]]))  # one unknown target
    rng = np.random.default_rng(3)
    u = ml_ds.users.ids()[5]
    hist = ml_ds.user_row(u)
    perm = rng.permutation(hist.ids())[:40]
    odd = np.concatenate([perm, perm[:2], [10 ** 9 + 1], perm[5:6], [10 ** 9 + 2]])
    queries = [RecQuery(user_id=u, user_items=hist),                    # a known user
               RecQuery(user_items=ItemList(item_ids=perm)),            # history only, unsorted
               RecQuery(user_items=ItemList(item_ids=odd))]             # repeats + unknown items
    refs = [hist.numbers(vocabulary=ml_ds.items), ml_ds.items.numbers(perm),
            ml_ds.items.numbers(odd, missing="negative")]
    peak = scorer.__class__(method="lift", damping=20, max_nbrs=1)
    peak.items, peak.item_freqs, peak.assoc_scores = scorer.items, scorer.item_freqs, \
        scorer.assoc_scores  # (the same learned state: its device copy is uploaded, not built)
    zeros = 0
    for q, r in zip(queries, refs):
        for comp, k in ((scorer, None), (peak, 1)):
            got = np.asarray(comp(q, all_items).scores(), np.float32)
            _assert_same(got[:n_items], R.scores(s, r, k), f"max_nbrs={k}")
            assert np.isnan(got[n_items])  # unknown target
            zeros += int((got[:n_items] == 0.0).sum())
    assert zeros > 0  # an unassociated target scores 0.0, not NaN
    # the order of the reference items is part of the contract
    assert not np.array_equal(_bits(R.scores(s, refs[1])), _bits(R.scores(s, refs[1][::-1])))
    # no reference items / only unknown ones: every score NaN
    for q in (RecQuery(user_id=-5), RecQuery(user_items=ItemList(item_ids=ids[:0])),
              RecQuery(user_items=ItemList(item_ids=[10 ** 9 + 1]))):
        for comp in (scorer, peak):
            assert np.isnan(np.asarray(comp(q, all_items).scores())).all()
    # score_batch = the per-query calls
    for il, r in zip(scorer.score_batch(queries, [all_items] * 3), refs):
        _assert_same(np.asarray(il.scores(), np.float32)[:n_items], R.scores(s, r))
    # other limits: the reference has no implementation; it raises once it has reference items
    five = AssociationScorer(method="lift", damping=20, max_nbrs=5)
    five.items, five.item_freqs, five.assoc_scores = scorer.items, scorer.item_freqs, \
        scorer.assoc_scores
    with pytest.raises(NotImplementedError):
        five(queries[0], all_items)
    with pytest.raises(NotImplementedError):
        five.recommend_batch(queries, 10)
    assert np.isnan(np.asarray(five(RecQuery(user_id=-5), all_items).scores())).all()

    # a pickle round trip keeps host state only and scores the same bits
    clone = pickle.loads(pickle.dumps(scorer))
    assert "_dev" not in clone.__dict__ and clone.is_trained()
    for q, r in zip(queries, refs):
        _assert_same(np.asarray(clone(q, all_items).scores(), np.float32)[:n_items],
                     R.scores(s, r))


def test_recommend_through_biased_lift_toml(gpu, oracle, ml_ds, ml_counts):
    from lkpy_amd import batch
    from lkpy_amd.data import RecQuery
    from lkpy_amd.knn import AssociationScorer
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "biased-lift.toml")
    pipe.train(ml_ds)
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, AssociationScorer) and scorer.config.method == "lift"
    s = R.train(*ml_counts, "lift", 20.0)
    assert np.array_equal(_bits(scorer.assoc_scores.data), _bits(s.data))
    n_items = s.shape[0]
    lens = np.diff(ml_ds._indptr)
    uids = ml_ds.users.ids()
    ends = [int(np.argmax(lens)), int(np.argmin(lens))]  # the longest and the shortest history
    pick = (ends + [i for i in range(0, len(uids), 10) if i not in ends])[:64]
    users = [int(uids[i]) for i in pick]
    assert len(users) == 64
    n = 10
    calls = []
    orig = pipe.run
    pipe.run = lambda *a, **k: (calls.append(a), orig(*a, **k))[1]
    got = batch.recommend(pipe, users, n)
    pipe.run = orig
    assert not calls, "batch.recommend must not fall back to one pipeline run per user"
    ties = 0
    for u in users:
        g = got.lookup(u)
        one = pipe.run("recommender", query=u, n=n)
        hist = ml_ds.user_row(u).numbers(vocabulary=ml_ds.items)
        row = R.scores(s, hist)
        widx, wsc = R.topn(row, hist, n, oracle.argtopn)
        for lst in (g, one):
            li = np.asarray(lst.numbers(vocabulary=scorer.items))
            ls = np.asarray(lst.scores(), np.float32)
            assert len(li) == n and len(np.unique(li)) == n and not np.isin(li, hist).any()
            assert np.array_equal(_bits(ls), _bits(wsc)), u  # position by position
            assert np.array_equal(_bits(row[li]), _bits(ls))  # an item carries its own score
            ties += int(not np.array_equal(li, widx))
    print(f"\n{len(users)} users x 2 paths: lists differing among bit-equal scores: {ties}")

    # the HistoryBatch path and the list-of-queries path give the same arrays; small panels too
    lookup = pipe.node("history-lookup").component
    with_unknown = users + [-7]
    gi, gs = scorer.recommend_batch(lookup.batch(with_unknown), n)
    li, ls = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in with_unknown], n)
    assert np.array_equal(gi, li) and np.array_equal(_bits(gs), _bits(ls))
    assert (gi[-1] == -1).all() and np.isnan(gs[-1]).all()  # the unknown user: nothing listed
    old = AssociationScorer.PANEL_BYTES
    try:
        AssociationScorer.PANEL_BYTES = 4 * n_items * 7  # panels of 7 queries
        pi, ps = scorer.recommend_batch(lookup.batch(with_unknown), n)
    finally:
        AssociationScorer.PANEL_BYTES = old
    assert np.array_equal(pi, gi) and np.array_equal(_bits(ps), _bits(gs))

    # dense_scores_batch rows = score_batch over all items
    from lkpy_amd.data import ItemList

    some = with_unknown[:6] + [-7]
    panel, valid, excl = scorer.dense_scores_batch(lookup.batch(some))
    panel = panel.cpu().numpy()
    assert panel.shape == (len(some), n_items) and valid.tolist() == [True] * 6 + [False]
    everything = ItemList(item_ids=ml_ds.items.ids())
    lists = scorer.score_batch([lookup(RecQuery.create(u)) for u in some],
                               [everything] * len(some))
    for r, il in enumerate(lists):
        _assert_same(panel[r], np.asarray(il.scores(), np.float32), f"panel row {r}")
    assert np.isnan(panel[-1]).all()
    own = [len(ml_ds.user_row(u)) for u in some[:6]]
    assert np.array_equal(np.diff(excl.indptr.cpu().numpy()), own + [0])

    # a stochastic ranker samples from the same panels: 4 lists per user, no history item in any
    pipe.replace_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                           query="history-lookup")
    many = batch.recommend_samples(pipe, users[:12], n, 4)
    assert many.key_fields == ("user_id", "sample") and len(many) == 48
    for u in users[:12]:
        own = ml_ds.user_row(u).ids()
        for k in range(4):
            il = many.lookup(u, k)
            assert len(il) == n and len(set(il.ids())) == n and not np.isin(il.ids(), own).any()


def test_score_batch_small_panels_equal_one_panel(gpu, monkeypatch, ml_ds, ml_lift20):
    """``score_batch`` through panels of 7 queries -- 8 of 7 and one of 6, the query without
    history in the last -- gives one panel's scores bit for bit: 62 queries, 40 targets each, one
    of them unknown."""
    from lkpy_amd import _device as D
    from lkpy_amd.basic import UserTrainingHistoryLookup
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.knn import AssociationScorer

    scorer, _s = ml_lift20
    lookup = UserTrainingHistoryLookup()
    lookup.train(ml_ds)
    users = list(ml_ds.users.ids()[:60]) + [int(ml_ds.users.ids()[-1]), -7]  # the last one unknown
    queries = [lookup(RecQuery.create(u)) for u in users]
    ids = ml_ds.items.ids()
    n_items = len(ids)
    rng = np.random.default_rng(11)
    lists, unknown_at = [], []
    for _ in users:
        unknown_at.append(int(rng.integers(0, 40)))
        lists.append(ItemList(item_ids=np.insert(rng.choice(ids, 39, replace=False),
                                                 unknown_at[-1], 10 ** 9)))
    assert len(queries) == 62 and scorer._panel_rows() >= 62
    one = scorer.score_batch(queries, lists)
    launched, score = [], D.assoc_score_batch
    with monkeypatch.context() as m:
        m.setattr(D, "assoc_score_batch",
                  lambda *a, **k: (launched.append(k.get("rows")), score(*a, **k))[1])
        m.setattr(AssociationScorer, "PANEL_BYTES", 4 * n_items * 7)  # panels of 7 queries
        small = scorer.score_batch(queries, lists)
    assert launched == [(lo, min(62, lo + 7)) for lo in range(0, 62, 7)] and len(launched) == 9
    assert [hi - lo for lo, hi in launched] == [7] * 8 + [6] and launched[-1] == (56, 62)
    assert len(one) == len(small) == 62
    finite = 0
    for a, b, il, at in zip(one, small, lists, unknown_at):
        assert np.array_equal(a.ids(), il.ids()) and np.array_equal(b.ids(), il.ids())
        sa, sb = np.asarray(a.scores(), np.float32), np.asarray(b.scores(), np.float32)
        assert sa.shape == (40,) and np.array_equal(_bits(sa), _bits(sb))
        assert np.isnan(sb[at])  # the unknown target
        finite += int(np.isfinite(sb).sum())
    assert np.isnan(np.asarray(small[-1].scores())).all()  # no reference items: every score NaN
    assert finite == 61 * 39  # every known target of a query with reference items has a score


def _small_dataset(seed, n_users, n_items):
    from lkpy_amd.data import Dataset

    rng = np.random.default_rng(seed)
    mat = sps.random_array((n_users, n_items), density=0.15, rng=rng, format="coo")
    item_ids = np.arange(100, 100 + n_items)
    return Dataset.from_arrays(mat.row + 1, item_ids[mat.col], all_item_ids=item_ids)


def test_full_ranking_and_retraining(gpu, oracle):
    """``n = None`` ranks every candidate (a 65-item vocabulary); after a retrain on other data the
    batch path must not score with the old model's device copy."""
    from lkpy_amd import batch
    from lkpy_amd.data import RecQuery
    from lkpy_amd.knn import AssociationScorer
    from lkpy_amd.pipeline import topn_pipeline

    first = _small_dataset(1, 40, 65)
    pipe = topn_pipeline(AssociationScorer(method="lift", damping=2.0))
    pipe.train(first)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    s = R.train(*R.cooc_counts(first.interaction_matrix()), "lift", 2.0)
    assert np.array_equal(_bits(scorer.assoc_scores.data), _bits(s.data))
    users = [int(u) for u in first.users.ids()]
    gi, gs = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in users], None)
    assert gi.shape == (len(users), 65)
    for r, u in enumerate(users):
        hist = first.user_row(u).numbers(vocabulary=first.items)
        widx, wsc = R.topn(R.scores(s, hist), hist, None, oracle.argtopn)
        k = 65 - len(np.unique(hist))
        assert len(widx) == k and (gi[r, k:] == -1).all() and np.isnan(gs[r, k:]).all()
        assert np.array_equal(_bits(gs[r, :k]), _bits(wsc))
        assert np.array_equal(np.sort(gi[r, :k]), np.setdiff1d(np.arange(65), hist))

    second = _small_dataset(2, 55, 90)
    pipe.train(second)  # Pipeline.train retrains trained components
    assert scorer.assoc_scores.shape == (90, 90)
    s2 = R.train(*R.cooc_counts(second.interaction_matrix()), "lift", 2.0)
    users = [int(u) for u in second.users.ids()]
    got = batch.recommend(pipe, users, 10)
    for u in users:
        g, one = got.lookup(u), pipe.run("recommender", query=u, n=10)
        hist = second.user_row(u).numbers(vocabulary=second.items)
        _widx, wsc = R.topn(R.scores(s2, hist), hist, 10, oracle.argtopn)
        assert np.array_equal(_bits(g.scores()), _bits(wsc))
        assert np.array_equal(_bits(one.scores()), _bits(wsc))
