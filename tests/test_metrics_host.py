"""CPU: the metrics restatement (``tests/metrics_restatement.py``) against closed forms worked out
by hand, the host side of ``lkpy_amd.metrics`` (rank weights, labels, packing, key matching, the
truth CSR) and the invariants of ``lkpy_amd.splitting`` on ml-latest-small."""
import math
import warnings
from pathlib import Path

import numpy as np
import pytest

import metrics_restatement as R

GOLDEN = Path(__file__).parent / "golden"
LG = math.log2


# ---- the restatement itself, on toy lists -------------------------------------------------

RECS = [10, 20, 30, 40, 50]  # hits at ranks 2 and 4
TEST = [20, 40, 99]


def test_restatement_binary_closed_forms():
    assert R.hit(RECS, TEST) == 1 and R.hit(RECS, TEST, 1) == 0
    assert R.recip_rank(RECS, TEST) == 0.5 and R.recip_rank(RECS, TEST, 1) == 0.0
    assert R.precision(RECS, TEST) == 2 / 5 and R.precision(RECS, TEST, 2) == 1 / 2
    assert R.recall(RECS, TEST) == 2 / 3
    assert R.recall(RECS, TEST, 2) == 1 / 2  # the denominator is min(len(test), n)
    # AP: (1/2 + 2/4) / min(3, 5)
    assert R.average_precision(RECS, TEST) == pytest.approx(1 / 3, rel=1e-15)
    assert R.average_precision(RECS, TEST, 2) == pytest.approx((1 / 2) / 2, rel=1e-15)
    # DCG, log2 weights clipped at rank 2: 1/lg2 + 1/lg4
    assert R.dcg(RECS, TEST) == pytest.approx(1.0 + 0.5, rel=1e-15)
    ideal = 1.0 + 1.0 + 1 / LG(3)
    assert R.ndcg(RECS, TEST) == pytest.approx(1.5 / ideal, rel=1e-15)
    assert R.ndcg(RECS, TEST, 2) == pytest.approx(1.0 / 2.0, rel=1e-15)  # ideal: fixed_dcg(2)
    # RBP, patience 0.85: (p + p^3) (1 - p)
    p = 0.85
    assert R.rbp(RECS, TEST) == pytest.approx((p + p ** 3) * (1 - p), rel=1e-14)
    # normalize: by the first min(n_test, len) = 3 weights
    assert R.rbp(RECS, TEST, normalize=True) == pytest.approx((p + p ** 3) / (1 + p + p * p),
                                                              rel=1e-14)
    # a weight without a series sum: by the weights of the list
    got = R.rbp(RECS, TEST, weight=R.log_weight, series_sum=None)
    assert got == pytest.approx(1.5 / (1 + 1 + 1 / LG(3) + 0.5 + 1 / LG(5)), rel=1e-15)


def test_restatement_corner_cases():
    nan = math.isnan
    for fn in (R.hit, R.recip_rank, R.rbp, R.dcg, R.ndcg, R.recall):
        assert nan(fn(RECS, [])), fn.__name__  # empty test list
    assert R.precision(RECS, []) == 0.0 and nan(R.precision([], TEST))
    assert nan(R.average_precision([], TEST))
    assert nan(R.average_precision(RECS, []))  # (ZeroDivisionError in the reference)
    assert R.hit([], TEST) == 0 and R.recip_rank([], TEST) == 0.0 and R.recall([], TEST) == 0.0
    assert R.ndcg([], TEST) == 0.0 and R.dcg([], TEST) == 0.0
    # a repeated recommended item counts every time
    assert R.precision([20, 20, 30], TEST) == 2 / 3
    assert R.int_stats([30, 20, 20], TEST) == (3, 2, 2)
    assert R.int_stats([30, 20, 20], TEST, 1) == (1, 0, 0)


def test_restatement_graded_closed_forms():
    gains = np.array([3.0, np.nan, -2.0], np.float32)  # 20 -> 3, 40 -> NaN, 99 -> clipped to 0
    # realized: only rank 2 (gain 3); rank 4's NaN gain is "not in the test data"
    assert R.dcg(RECS, TEST, gains=gains) == pytest.approx(3.0, rel=1e-15)
    # ideal: [3, 0] . [1, 1]
    assert R.ndcg(RECS, TEST, gains=gains) == pytest.approx(1.0, rel=1e-15)
    g2 = np.array([1.0, 4.0, 2.0], np.float32)
    # realized 1/1 + 4/2; ideal 4 + 2 + 1/lg3
    assert R.ndcg(RECS, TEST, gains=g2) == pytest.approx(3.0 / (6 + 1 / LG(3)), rel=1e-15)
    assert R.ndcg(RECS, TEST, 1, gains=g2) == 0.0 / 4.0
    assert R.ndcg(RECS, TEST, 2, gains=g2) == pytest.approx(1.0 / 6.0, rel=1e-15)
    assert math.isnan(R.ndcg(RECS, TEST, gains=np.full(3, np.nan, np.float32)))
    assert R.ndcg(RECS, TEST, gains=np.array([0, -1, 0], np.float32)) == 0.0  # ideal 0


def test_restatement_predict_errors_and_stats():
    sse, sae, n, ms, mt = R.predict_errors([1, 2, 3, 4], [3.0, np.nan, 2.5, 1.0],
                                           [3, 1, 2, 9], [2.0, 3.5, 4.0, np.nan])
    # pairs: 1 -> (3.0, 3.5), 3 -> (2.5, 2.0); 2 is scored NaN (missing score), 9 has a NaN
    # rating; 4 is scored without truth
    assert (sse, sae, n, ms, mt) == (0.5, 1.0, 2, 1, 1)
    st = R.value_stats([1.0, np.nan, 3.0, None])
    assert st == {"n": 2, "mean": 2.0, "median": 2.0, "std": 1.0}


# ---- the metric classes' host side -----------------------------------------------------------


def test_rank_weight_tables_equal_the_formulas():
    from lkpy_amd import metrics as M

    ranks = np.arange(1, 301)
    assert np.array_equal(M.LogRankWeight().weight(ranks), R.log_weight(ranks))
    assert np.array_equal(M.LogRankWeight(base=10, offset=1).weight(ranks),
                          np.log(10) / np.log(ranks + 1))
    assert M.LogRankWeight().weight(np.array([1, 2, 4]))[1:].tolist() == [1.0, 0.5]
    assert M.LogRankWeight().weight(np.array([1]))[0] == 1.0  # ranks clipped at 2
    g = M.GeometricRankWeight(0.5)
    assert np.array_equal(g.weight(ranks), np.exp(np.log(0.5) * (ranks - 1)))
    assert np.allclose(g.weight(ranks[:4]), [1, 0.5, 0.25, 0.125], rtol=1e-15)
    assert g.series_sum() == 2.0 and M.LogRankWeight().series_sum() is None
    assert np.array_equal(g.log_weight(ranks), np.log(0.5) * (ranks - 1))
    assert np.array_equal(M.LogRankWeight().log_weight(ranks), np.log(R.log_weight(ranks)))
    with pytest.raises(ValueError):
        M.GeometricRankWeight(1.0)


def test_labels_alias_and_validation():
    from lkpy_amd import metrics as M

    assert M.NDCG(10).label == "NDCG@10" and M.NDCG().label == "NDCG"
    assert [c(5).label for c in (M.Hit, M.RecipRank, M.Precision, M.Recall, M.AveragePrecision,
                                 M.DCG, M.RBP)] == \
        ["Hit@5", "RecipRank@5", "Precision@5", "Recall@5", "AveragePrecision@5", "DCG@5",
         "RBP@5"]
    assert M.RMSE().label == "RMSE" and M.MAE().label == "MAE"
    with pytest.warns(DeprecationWarning):
        m = M.Recall(k=7)
    assert m.n == 7 and m.k == 7
    with pytest.raises(ValueError):
        M.Hit(-1)
    assert M.Hit.default == 0.0 and M.RMSE.default is None
    mc = M.MeasurementCollector()
    mc.add_metric(M.NDCG)
    mc.add_metric(M.NDCG(5))
    mc.add_metric(lambda out, test: 1.0, "one")
    assert mc.metric_names == ["NDCG", "NDCG@5", "one"]
    with pytest.raises(RuntimeError, match="duplicate"):
        mc.add_metric(M.NDCG())
    assert mc.empty_copy().metric_names == mc.metric_names


def test_rank_plan_collects_cutoffs_tables_and_ideals():
    from lkpy_amd import metrics as M

    plan = M._RankPlan()
    geo = M.GeometricRankWeight(0.85)
    for m in (M.Hit(), M.Hit(5), M.NDCG(5), M.NDCG(gain="rating"), M.RBP(), M.RBP(weight=geo),
              M.DCG(0)):
        m._request(plan)
    assert plan.cutoffs == [0, 5]  # None -> 0 (whole list); n = 0 needs no statistics
    assert list(plan.weights) == [("log", 2, 0), ("geometric", 0.85)]
    assert plan.gains == ["rating"] and plan.ideals == [(0, ("log", 2, 0), "rating")]


# ---- packing, key projection, the truth CSR ----------------------------------------------------


def _three_lists():
    from lkpy_amd.data import ItemList, ItemListCollection, Vocabulary

    vocab = Vocabulary(np.array([5, 7, 11, 13, 17]), "item")
    nums = np.array([[4, 0, 2], [1, 3, -1], [-1, -1, -1]], np.int32)
    scores = np.array([[3, 2, 1], [2, 1, np.nan], [np.nan] * 3], np.float32)
    users = np.array([30, 10, 20])
    arr = ItemListCollection.from_arrays(users, nums, scores, vocab)
    lst = ItemListCollection(("user_id",))
    for u, r, s in zip(users, nums, scores):
        lst.add(ItemList(item_nums=r[r >= 0], vocabulary=vocab, scores=s[r >= 0], ordered=True),
                int(u))
    return vocab, users, nums, arr, lst


def test_list_backed_and_array_backed_collections_pack_alike():
    from lkpy_amd import metrics as M

    vocab, users, nums, arr, lst = _three_lists()
    pa, pl = M.pack_collection(arr), M.pack_collection(lst)
    assert pa.dense is not None and pl.ragged is not None
    da, _ = M.dense_lists(pa, vocab)
    dl, _ = M.dense_lists(pl, vocab)
    assert da.dtype == dl.dtype == np.int32 and np.array_equal(da, dl) and np.array_equal(da, nums)
    assert np.array_equal(pa.key_columns()["user_id"], pl.key_columns()["user_id"])
    for a, b in zip(pa.as_ragged(), M._Packed(pl.keys, pl.key_fields, dense=(dl, vocab),
                                              scores=arr._lists.scores).as_ragged()):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b)
    assert not arr._lists._made  # no ItemList was built from the arrays
    # an id the vocabulary does not know keeps its rank
    from lkpy_amd.data import ItemList, ItemListCollection

    c = ItemListCollection(("user_id",))
    c.add(ItemList([7, 999, 5], ordered=True), 1)
    d, _ = M.dense_lists(M.pack_collection(c), vocab)
    assert d.tolist() == [[1, int(M.UNKNOWN_ITEM), 0]]


def test_truth_csr_sorted_duplicate_free_and_key_projection():
    from lkpy_amd import metrics as M
    from lkpy_amd.data import ItemListCollection, Vocabulary

    vocab = Vocabulary(np.array([5, 7, 11, 13, 17]), "item")
    # user 10: items out of order with a repeat and an unknown id; user 20: empty
    offsets = np.array([0, 5, 5, 7])
    ids = np.array([13, 5, 13, 999, 7, 17, 11])
    rating = np.array([1, 2, 3, 4, 5, 6, 7], np.float32)
    test = ItemListCollection.from_ragged(np.array([10, 20, 30]), offsets, ids,
                                          {"rating": rating})
    ts = M.truth_state(test, vocab)
    assert ts is M.truth_state(test, vocab)  # built once per (collection, vocabulary)
    assert ts.lens.tolist() == [5, 0, 2]  # len(test): every item, repeated and unknown too
    assert ts.indptr.tolist() == [0, 4, 4, 6]
    assert ts.indices.tolist() == [0, 1, 3, 5, 2, 4]  # ascending; 999 numbered past the vocabulary
    for r in range(3):
        row = ts.indices[ts.indptr[r]:ts.indptr[r + 1]]
        assert np.all(np.diff(row) > 0)
    assert ts.values("rating").tolist() == [2, 5, 1, 4, 7, 6]  # (the first of equal items)
    with pytest.raises(KeyError):
        ts.values("gain")
    # output keys with two fields, projected onto the test collection's one
    keys = {"user_id": np.array([30, 10, 77, 10]), "run": np.array([0, 0, 1, 1])}
    assert ts.match(keys, 4).tolist() == [2, 0, -1, 0]
    with pytest.raises(KeyError):
        ts.match({"run": keys["run"]}, 4)
    # without a vocabulary the test items number themselves
    own = M.truth_state(test)
    assert own.vocab.ids().tolist() == [5, 7, 11, 13, 17, 999] and own.lens.tolist() == [5, 0, 2]
    # of equal test keys the last wins, as ``lookup`` does
    dup = ItemListCollection.from_ragged(np.array([1, 1]), np.array([0, 1, 2]), np.array([5, 7]))
    assert M.truth_state(dup).match({"user_id": np.array([1])}, 1).tolist() == [1]


def test_lookup_projected_and_itemlist_helpers():
    from collections import namedtuple

    from lkpy_amd.data import ItemList, ItemListCollection

    c = ItemListCollection(("user_id",))
    il = ItemList([3, 4, 5], scores=[3.0, 2.0, 1.0], ordered=True)
    c.add(il, 9)
    K = namedtuple("K", ["user_id", "run"])
    assert c.lookup_projected(K(9, 2)) is il and c.lookup_projected(K(8, 2)) is None
    assert il[:2].ids().tolist() == [3, 4] and il[:2].ordered
    assert il[np.array([2, 0])].scores().tolist() == [1.0, 3.0]
    assert il.isin(ItemList([5, 3])).tolist() == [True, False, True]
    assert il.ranks().tolist() == [1, 2, 3] and ItemList([1]).ranks() is None


def test_metrics_need_the_device():
    "no host-only implementation: without a GPU a measurement raises, it does not fall back"
    import torch

    from lkpy_amd import _native
    from lkpy_amd import metrics as M
    from lkpy_amd.data import ItemList

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_native.BackendUnavailable):
        M.Hit().measure_list(ItemList([1, 2], ordered=True), ItemList([2]))


# ---- splitting ----------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _pairs(ds):
    return set(zip(ds._rows.tolist(), ds._cols.tolist()))


def _check_split(ds, split, users_expected, size_of):
    test = split.test
    ll = test._lists
    users = np.asarray(ll.raw_keys)
    assert len(users) == users_expected and len(np.unique(users)) == len(users)
    lens = np.diff(ll.offsets)
    unums = ds.users.numbers(users)
    row_len = np.diff(ds._indptr)[unums]
    assert lens.tolist() == [size_of(int(n)) for n in row_len]
    t_pairs = set(zip(np.repeat(unums, lens).tolist(), ds.items.numbers(ll.item_ids).tolist()))
    assert len(t_pairs) == int(lens.sum()) == split.test_size
    tr = _pairs(split.train)
    assert not (tr & t_pairs) and (tr | t_pairs) == _pairs(ds)
    assert split.train.users is ds.users and split.train.items is ds.items
    assert set(ll.fields) == set(ds._attrs)
    # the lists carry the rows' own ratings
    want = {(u, i): r for u, i, r in zip(ds._rows.tolist(), ds._cols.tolist(),
                                         ds._attrs["rating"].tolist())}
    got = ll.fields["rating"].tolist()
    for (u, i), r in zip(zip(np.repeat(unums, lens).tolist(),
                             ds.items.numbers(ll.item_ids).tolist()), got):
        assert want[(u, i)] == r
    return users


def test_sample_users_invariants(ml_ds):
    from lkpy_amd.splitting import SampleFrac, SampleN, TTSplit, sample_users

    split = sample_users(ml_ds, 134, SampleFrac(0.2, rng=3), rng=3)
    assert isinstance(split, TTSplit)
    users = _check_split(ml_ds, split, 134, lambda n: round(n * 0.2))
    again = sample_users(ml_ds, 134, SampleFrac(0.2, rng=3), rng=3)
    assert np.array_equal(np.asarray(again.test._lists.raw_keys), users)
    assert np.array_equal(again.test._lists.item_ids, split.test._lists.item_ids)
    other = sample_users(ml_ds, 134, SampleFrac(0.2, rng=4), rng=4)
    assert not np.array_equal(np.asarray(other.test._lists.raw_keys), users)
    _check_split(ml_ds, sample_users(ml_ds, 50, SampleN(5, rng=1), rng=1), 50,
                 lambda n: min(5, n))
    # the generator is used as the reference uses it: one choice of users, then one per user
    rng = np.random.default_rng(3)
    assert np.array_equal(rng.choice(ml_ds.users.ids(), 134, replace=False), users)
    # repeats: an iterator of disjoint samples
    parts = list(sample_users(ml_ds, 100, SampleN(3, rng=1), repeats=3, rng=5))
    seen = np.concatenate([np.asarray(p.test._lists.raw_keys) for p in parts])
    assert len(parts) == 3 and len(np.unique(seen)) == 300


def test_last_n_and_last_frac_take_the_largest_values(ml_ds):
    from lkpy_amd.data import Dataset
    from lkpy_amd.splitting import LastFrac, LastN, sample_users

    rng = np.random.default_rng(11)
    stamp = rng.permutation(ml_ds.interaction_count).astype(np.int64)  # a synthetic ordering
    ds = Dataset(ml_ds.users, ml_ds.items, ml_ds._rows, ml_ds._cols,
                 {"rating": ml_ds._attrs["rating"], "timestamp": stamp})
    for method, size_of in ((LastN(4), lambda n: min(4, n)),
                            (LastFrac(0.25), lambda n: round(n * 0.25))):
        split = sample_users(ds, 60, method, rng=2)
        ll = split.test._lists
        users = np.asarray(ll.raw_keys)
        assert len(users) == 60
        for i, u in enumerate(ds.users.numbers(users).tolist()):
            s, e = int(ds._indptr[u]), int(ds._indptr[u + 1])
            k = size_of(e - s)
            mine = np.sort(ll.fields["timestamp"][int(ll.offsets[i]):int(ll.offsets[i + 1])])
            assert len(mine) == k
            assert np.array_equal(mine, np.sort(ds._attrs["timestamp"][s:e])[e - s - k:])
    with pytest.raises(TypeError):
        sample_users(ml_ds, 5, LastN(2), rng=1)  # the fixture has no timestamps


def test_crossfold_users_partitions_the_users(ml_ds):
    from lkpy_amd.splitting import SampleN, crossfold_users

    folds = list(crossfold_users(ml_ds, 5, SampleN(5, rng=9), rng=9))
    assert len(folds) == 5
    users = [np.asarray(f.test._lists.raw_keys) for f in folds]
    assert sorted(len(u) for u in users) == sorted(len(p) for p in
                                                   np.array_split(np.arange(ml_ds.user_count), 5))
    allu = np.concatenate(users)
    assert np.array_equal(np.sort(allu), np.sort(ml_ds.users.ids()))
    _check_split(ml_ds, folds[0], len(users[0]), lambda n: min(5, n))
    only = next(crossfold_users(ml_ds, 5, SampleN(5, rng=9), test_only=True, rng=9))
    assert only.train.interaction_count == 0 and only.train.items is ml_ds.items
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(np.asarray(only.test._lists.raw_keys), users[0])
