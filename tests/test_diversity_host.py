"""CPU: the restatement ``tests/diversity_restatement.py`` on hand-checkable cases, and the
host-side argument handling of the exposure / diversity / popularity / reranking metrics
(labels, ``k=``, the category limit, matrix normalisation, key projection)."""
import math
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

import diversity_restatement as R


def test_restatement_gini():
    assert R.gini([0, 0, 1]) == pytest.approx(2 / 3, abs=1e-15)
    assert R.gini([3.0, 3.0, 3.0, 3.0]) == 0
    tot = R.exposure_totals([np.array([0, 2, 9, -1]), np.array([2, 1])], 4)
    assert tot.tolist() == [1.0, 1.0, 2.0, 0.0]
    geo = R.exposure_totals([np.array([0, 2]), np.array([2, 1])], 3, n=1, weight=R.geometric_weight)
    assert geo.tolist() == [1.0, 0.0, 1.0]


def test_restatement_ils_and_entropy():
    same = R.normalize_rows(np.array([[2.0, 0, 0]] * 3), "unit")
    assert R.ils(np.arange(3), same) == 1.0
    assert R.ils(np.arange(3), np.eye(3)) == 0.0
    assert R.ils(np.array([1]), np.eye(3)) == 1.0 and math.isnan(R.ils(np.array([7]), np.eye(3)))
    assert math.isnan(R.ils(np.zeros(0, int), np.eye(3)))
    # k of C categories equally filled by m items each: the smoothed closed form
    C, k, m = 6, 3, 2
    dist = np.zeros((k * m, C))
    dist[np.arange(k * m), np.arange(k * m) % k] = 1.0
    tot = k * (m + 1e-6) + (C - k) * 1e-6
    p, q = (m + 1e-6) / tot, 1e-6 / tot
    want = -(k * p * math.log2(p) + (C - k) * q * math.log2(q))
    assert R.entropy(np.arange(k * m), dist) == pytest.approx(want, abs=1e-14)
    assert math.isnan(R.entropy(np.array([99]), dist))


def test_restatement_rbo_and_lip():
    a = np.arange(10)
    assert R.rbo(a, a) == pytest.approx(1.0, abs=1e-15)
    assert R.rbo(a, a + 100) == 0
    # a list shorter than n: the overlap stays 2 and is still divided by d
    s, t = R.rbo_sum(np.array([1, 2]), np.array([2, 1]), np.ones(4))
    assert s == 0 / 1 + 2 / 2 + 2 / 3 + 2 / 4 and t == 4
    assert R.lip(np.arange(50), np.array([3, 1, 2]), n=3) == 0
    assert R.lip(np.arange(50), np.array([3, 41, 2]), n=3) == 41 - 3
    assert math.isnan(R.lip(np.zeros(0, int), np.array([1]), n=3))


def test_restatement_pop_table_and_the_product_table():
    from lkpy_amd import metrics as M
    from lkpy_amd.data import Dataset

    # five items: counts 3, 1, 3, 0, 2 -- a tie and an item nobody has
    table = R.pop_table([3, 1, 3, 0, 2])
    assert table.tolist() == [3.5 / 4, 1 / 4, 3.5 / 4, 0.0, 2 / 4]
    users = [0, 1, 2, 0, 0, 1, 2, 3, 4, 0]
    items = [10, 10, 10, 11, 12, 12, 12, 14, 14, 10]  # (0, 10) twice: one user
    ds = Dataset.from_arrays(users, items, all_item_ids=[10, 11, 12, 13, 14])
    assert np.array_equal(M.popularity_quantiles(ds, "users"), table)
    assert np.array_equal(M.popularity_quantiles(ds, "interactions"),
                          R.pop_table([4, 1, 3, 0, 2]))
    assert R.mean_pop_rank(np.array([0, 3, 99]), table) == pytest.approx(3.5 / 12)
    assert math.isnan(R.mean_pop_rank(np.zeros(0, int), table))


def test_stats_gini_and_its_warnings():
    from lkpy_amd.knn import DataWarning
    from lkpy_amd.stats import gini

    rng = np.random.default_rng(3)
    x = rng.random(101)
    assert gini(x) == R.gini(x)
    assert gini([0, 0, 1]) == pytest.approx(2 / 3, abs=1e-15) and gini(np.ones(5)) == 0
    with pytest.warns(DataWarning, match="negative"):
        gini([-1.0, 2.0, 3.0])
    with pytest.warns(DataWarning, match="non-positive"):
        gini(np.zeros(4))


def test_labels_cutoffs_and_constructor_forms():
    from lkpy_amd import metrics as M
    from lkpy_amd.data import Dataset, Vocabulary

    vocab = Vocabulary(np.arange(100, 106))
    cats = np.arange(18, dtype=float).reshape(6, 3)
    assert M.ListGini(10, items=vocab).label == "ListGini@10"
    assert M.ExposureGini(items=vocab).label == "ExposureGini"
    assert M.ExposureGini(items=vocab).weight.patience == 0.85
    with pytest.warns(DeprecationWarning):
        assert M.ListGini(k=5, items=vocab).n == 5
    ds = Dataset.from_arrays([1, 2], [100, 105], all_item_ids=vocab.ids())
    assert M.ListGini(items=ds).item_vocab is ds.items
    with pytest.warns(DeprecationWarning):
        assert M.MeanPopRank(ds, k=7).label == "MeanPopRank@7"
    with pytest.raises(ValueError):
        M.MeanPopRank(ds, count="clicks")
    ds.item_attrs["genre"] = cats
    assert M.ILS(ds, "genre", 10).label == "ILS(genre)@10"
    assert M.Entropy(ds, "genre").label == "Entropy(genre)"
    rbe = M.RankBiasedEntropy(ds, "genre", 5)
    assert rbe.label == "RBEntropy(genre)@5" and rbe.weight.patience == 0.85
    assert M.ILS(categories=cats, items=vocab, attribute="tag", n=3).label == "ILS(tag)@3"
    with pytest.raises(KeyError):
        M.ILS(ds, "tag")
    with pytest.raises(TypeError):
        M.ILS(categories=cats)
    with pytest.raises(ValueError, match="rows"):
        M.ILS(categories=cats[:4], items=vocab)
    for m in (M.ListGini(items=vocab), M.ExposureGini(items=vocab)):
        assert m.extract_list_metrics((np.arange(2), 1.0)) is None
    assert pickle.loads(pickle.dumps(rbe)).label == rbe.label


def test_gini_measure_list_intermediates():
    from lkpy_amd import metrics as M
    from lkpy_amd.data import ItemList, Vocabulary

    vocab = Vocabulary(np.arange(100, 106))
    il = ItemList(item_ids=[105, 100, 103], ordered=True)
    ids, w = M.ListGini(2, items=vocab).measure_list(il, None)
    assert ids.tolist() == [5, 0] and w == 1.0
    ids, w = M.ExposureGini(items=vocab).measure_list(il, None)
    assert ids.tolist() == [5, 0, 3]
    assert np.array_equal(w, R.geometric_weight(np.arange(1, 4)))


def test_category_limit_is_a_value_error_that_names_it():
    from lkpy_amd import _device as D
    from lkpy_amd import _native
    from lkpy_amd import metrics as M
    from lkpy_amd.data import Vocabulary

    assert D.CATEGORY_MAX == _native.load(build_if_missing=True).lk_list_category_max() >= 4096
    vocab = Vocabulary(np.arange(3))
    M.Entropy(categories=sps.csr_array((3, D.CATEGORY_MAX)), items=vocab)
    for form in (sps.csr_array((3, D.CATEGORY_MAX + 1)), np.zeros((3, D.CATEGORY_MAX + 1))):
        with pytest.raises(ValueError, match=str(D.CATEGORY_MAX)):
            M.Entropy(categories=form, items=vocab)


@pytest.mark.parametrize("mode", ["unit", "distribution"])
def test_normalize_rows_dense_and_sparse(mode):
    from lkpy_amd import metrics as M

    rng = np.random.default_rng(11)
    dense = rng.random((7, 5)) * (rng.random((7, 5)) < 0.5)
    dense[3] = 0.0  # a row of zeros stays
    want = R.normalize_rows(dense, mode)
    got = M.normalize_rows(dense, mode)
    assert isinstance(got, np.ndarray) and np.allclose(got, want, rtol=0, atol=1e-15)
    for form in (sps.csr_array, sps.coo_array, sps.csc_matrix):
        sp = M.normalize_rows(form(dense), mode)
        assert isinstance(sp, sps.csr_array) and sp.dtype == np.float64
        assert np.allclose(sp.toarray(), want, rtol=0, atol=1e-15)
    assert np.all(got[3] == 0)
    if mode == "distribution":
        with pytest.raises(ValueError, match="negative"):
            M.normalize_rows(-dense, mode)


def test_key_projection_of_sample_keys_onto_user_keys():
    from lkpy_amd import metrics as M

    ref_keys = {"user_id": np.array([7, 3, 9, 3])}  # of the two lists of user 3 the last wins
    index = M.key_index(("user_id",), ref_keys)
    out = {"user_id": np.array([3, 3, 5, 9, 7]), "sample": np.array([0, 1, 0, 0, 2])}
    assert M.project_rows(index, ("user_id",), out, 5).tolist() == [3, 3, -1, 2, 0]
    with pytest.raises(KeyError, match="reference"):
        M.project_rows(index, ("user_id",), {"sample": out["sample"]}, 5, "reference")
    two = M.key_index(("user_id", "part"), {"user_id": np.array([1, 1]), "part": np.array([0, 1])})
    probe = {"user_id": np.array([1, 1, 2]), "part": np.array([1, 0, 0]), "sample": np.zeros(3)}
    assert M.project_rows(two, ("user_id", "part"), probe, 3).tolist() == [1, 0, -1]


def test_reranking_depth_is_checked_before_any_device_work():
    from lkpy_amd import reranking_metrics as RM
    from lkpy_amd.data import ItemList

    a = ItemList(item_ids=[1, 2, 3], ordered=True)
    for n in (0, 1025):
        with pytest.raises(ValueError, match="1024"):
            RM.rank_biased_overlap(a, a, n=n)
        with pytest.raises(ValueError, match="1024"):
            RM.least_item_promoted(a, a, n=n)


def test_new_entry_points_validate_arguments_without_a_gpu():
    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    assert lib.lk_item_exposure_workspace_bytes(0, 10) == 0
    assert lib.lk_item_exposure_workspace_bytes(70, 64) >= 6 * 4 * 70 * 64
    assert lib.lk_item_exposure(None, 3, 4, 5, 0, None, 0, 7, None, None, None) == \
        _native.LK_E_INVALID and b"shape" in lib.lk_last_error()
    assert lib.lk_list_category_stats(None, 1, 4, 4, 0, 7, None, None, None, 7169, None, 0, None,
                                      None, None) == _native.LK_E_INVALID
    assert b"7168" in lib.lk_last_error()
    assert lib.lk_list_pair_stats(1, None, None, None, None, None, 1025, None, None, None, None,
                                  None) == _native.LK_E_INVALID
    assert b"1024" in lib.lk_last_error()
    assert lib.lk_list_gather_mean(None, 1, 4, 5, 0, None, 0, None, None, None) == \
        _native.LK_E_INVALID
