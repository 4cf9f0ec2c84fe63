"""GPU: the exposure / diversity / popularity / reranking metrics (csrc/diversity.hip +
``lkpy_amd.metrics``, ``lkpy_amd.reranking_metrics``) against ``tests/diversity_restatement.py``.

Bars: the exposure totals, the Gini summaries made of them, RBO's agreement sum and LIP are
BIT-identical to the restatement (the device adds in the restatement's order).  ILS is within
1e-10 absolute (the float64 error of the column-sum identity is about
``2 (C + n + 4) 2**-53 n / (n - 1)``, below 1e-11 at C = 16 384, n = 1000), an entropy within
``1e-10 log2(C + 1)`` (a few ulp per term over C terms), a popularity mean within ``n 2**-53``
(table values in [0, 1]; NumPy's pairwise order against the rank order)."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

import diversity_restatement as R

pytestmark = pytest.mark.gpu
UNKNOWN = 0x7FFFFFFF
U = 2.0 ** -53


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def _dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _rows(panel):
    "the lists of a -1 padded panel without their padding"
    return [r[r >= 0] for r in panel]


# ---- exposure --------------------------------------------------------------------------------


def _exposure(gpu, panels, n_items, cutoff, weight, ld_weights):
    "the device totals after feeding ``panels`` one call after the other"
    import torch

    from lkpy_amd import _device as D

    totals = torch.zeros(n_items, dtype=torch.float64, device=gpu)
    w = None if weight is None else _dev(weight(np.arange(1, ld_weights + 1)), gpu)
    for p in panels:
        D.item_exposure(_dev(p.astype(np.int32), gpu), totals, cutoff, w)
    return totals.cpu().numpy()


@pytest.mark.parametrize("weight", [None, R.geometric_weight])
def test_exposure_small_with_padding_empty_list_and_cutoff(gpu, weight):
    panel = np.array([[3, -1, 0, 6, 2],
                      [-1, -1, -1, -1, -1],
                      [6, UNKNOWN, 3, -1, 1]], np.int32)
    for cutoff in (0, 3, 1):
        got = _exposure(gpu, [panel], 7, cutoff, weight, 5)
        want = R.exposure_totals(_rows(panel), 7, cutoff or None, weight)
        assert np.array_equal(_bits(got), _bits(want)), cutoff
    assert want[4] == 0 and want[5] == 0


@pytest.mark.parametrize("weight", [None, R.geometric_weight])
def test_exposure_across_sort_tiles_and_however_the_lists_are_fed(gpu, weight):
    "70 x 64 = 4480 entries > one 4096-key sort tile; item 0 in every list, item 299 in none"
    rng = np.random.default_rng(5)
    n_items = 300
    panel = np.empty((70, 64), np.int32)
    for q in range(70):
        row = np.append(rng.choice(np.arange(1, n_items - 1), 63, replace=False), 0)
        panel[q] = rng.permutation(row)
    want = R.exposure_totals(list(panel), n_items, None, weight)
    assert want[n_items - 1] == 0 and (weight is not None or want[0] == 70)
    one = _exposure(gpu, [panel], n_items, 0, weight, 64)
    two = _exposure(gpu, [panel[:30], panel[30:]], n_items, 0, weight, 64)
    each = _exposure(gpu, [panel[q:q + 1] for q in range(70)], n_items, 0, weight, 64)
    for got in (one, two, each):
        assert np.array_equal(_bits(got), _bits(want))


def test_gini_summaries_are_the_host_expression_on_the_same_totals(gpu):
    from lkpy_amd import metrics as M
    from lkpy_amd.data import ItemList, ItemListCollection, Vocabulary

    rng = np.random.default_rng(6)
    vocab = Vocabulary(np.arange(1000, 1200))
    panel = np.stack([rng.choice(200, 30, replace=False) for _ in range(50)]).astype(np.int32)
    panel[7, 20:] = -1
    users = np.arange(50)
    test = ItemListCollection.from_dict({0: ItemList(item_ids=[1000])}, key=("user_id",))
    want = {}
    for lbl, n, w in (("ListGini", None, None), ("ExposureGini@10", 10, R.geometric_weight)):
        want[lbl] = R.gini_of_totals(R.exposure_totals(_rows(panel), 200, n, w))

    def collector():
        mc = M.MeasurementCollector()
        mc.add_metric(M.ListGini(items=vocab))
        mc.add_metric(M.ExposureGini(10, items=vocab))
        return mc

    whole, parts = collector(), collector()
    whole.add_array_measurements(users, panel, test, vocabulary=vocab)
    parts.add_array_measurements(users[:20], panel[:20], test, vocabulary=vocab)
    parts.add_array_measurements(users[20:], _dev(panel[20:], gpu), test, vocabulary=vocab)
    for mc in (whole, parts):
        summary = mc.summary_metrics()
        assert set(summary) == set(want) and list(mc.list_metrics().columns) == []
        for lbl in want:
            assert _bits(summary[lbl]) == _bits(want[lbl]), lbl
    fresh = parts.empty_copy()
    parts.reset()
    for mc in (fresh, parts):  # no totals are carried over
        mc.add_array_measurements(users, panel, test, vocabulary=vocab)
        assert _bits(mc.summary_metrics()["ListGini"]) == _bits(want["ListGini"])
    # the lists numbered by ANOTHER vocabulary: renumbered on the device, unknown items skipped
    other = Vocabulary(np.arange(1100, 1300))
    mc = collector()
    mc.add_array_measurements(users, panel, test, vocabulary=other)
    moved = [np.where(r + 100 < 200, r + 100, UNKNOWN) for r in _rows(panel)]
    assert _bits(mc.summary_metrics()["ListGini"]) == \
        _bits(R.gini_of_totals(R.exposure_totals(moved, 200)))


# ---- category statistics ---------------------------------------------------------------------

N_CAT_ITEMS = 150


def _category_lists():
    "lists of 0, 1, 2 and 100 known items, one with unknown items and gaps, one of unknown only"
    rng = np.random.default_rng(8)
    panel = np.full((6, 110), -1, np.int32)
    panel[1, 0] = 17
    panel[2, :2] = (3, 149)
    panel[3, :100] = rng.choice(N_CAT_ITEMS, 100, replace=False)
    mixed = rng.choice(N_CAT_ITEMS, 40, replace=False).astype(np.int32)
    mixed[[0, 5, 39]] = (UNKNOWN, N_CAT_ITEMS + 3, UNKNOWN)
    panel[4, :50] = -1
    panel[4, 3:83:2] = mixed
    panel[5, :3] = (UNKNOWN, N_CAT_ITEMS, UNKNOWN)
    return panel


def _category_matrix(C):
    rng = np.random.default_rng(100 + C)
    m = rng.random((N_CAT_ITEMS, C)) * (rng.random((N_CAT_ITEMS, C)) < min(1.0, 6 / C))
    m[11] = 0.0  # an item without any category
    return m


@pytest.fixture(scope="module")
def category_reference():
    "restatement values per C: computed once, shared by the dense and the sparse run"
    out = {}
    for C in (1, 20, 65, 7168):
        m = _category_matrix(C)
        unit, dist = R.normalize_rows(m, "unit"), R.normalize_rows(m, "distribution")
        rows = _rows(_category_lists())
        out[C] = {(name, n): np.array([f(r, n) for r in rows]) for n in (None, 50) for name, f in (
            ("ils", lambda r, n: R.ils(r, unit, n)),
            ("ent", lambda r, n: R.entropy(r, dist, n)),
            ("rbe", lambda r, n: R.entropy(r, dist, n, R.geometric_weight)))}
    return out


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("C", [1, 20, 65, 7168])
def test_category_stats(gpu, category_reference, C, sparse):
    from lkpy_amd import _device as D
    from lkpy_amd import metrics as M
    from lkpy_amd.data import Vocabulary

    assert D.CATEGORY_MAX == 7168
    m = _category_matrix(C)
    cats = sps.coo_array(m) if sparse else m
    vocab = Vocabulary(np.arange(N_CAT_ITEMS))
    panel = _category_lists()
    packed = M._Packed(np.arange(len(panel)), ("list",), dense=(panel, vocab))
    ms, names = [], []
    for n in (None, 50):
        ms += [M.ILS(categories=cats, items=vocab, n=n), M.Entropy(categories=cats, items=vocab, n=n),
               M.RankBiasedEntropy(categories=cats, items=vocab, n=n)]
        names += [("ils", n), ("ent", n), ("rbe", n)]
    vals, _extras, _ = M.measure_arrays(ms, packed, None)
    for (name, n), got in zip(names, vals):
        want = category_reference[C][(name, n)]
        print(C, sparse, name, n, "max abs diff", np.nanmax(np.abs(got - want)))
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, n)
        assert np.isnan(got[[0, 5]]).all() and not np.isnan(got[1:5]).any()
        tol = 1e-10 if name == "ils" else 1e-10 * math.log2(C + 1)
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= tol), (name, n, got, want)
        if name == "ils":
            assert got[1] == 1.0  # one known item, exactly


def test_category_raw_outputs_against_the_literal_triangle(gpu):
    "sq_sum / self_sum of lk_list_category_stats: (sq - self) / 2 is sum(triu(V V^T, 1))"
    from lkpy_amd import _device as D

    C = 65
    unit = R.normalize_rows(_category_matrix(C), "unit")
    panel = _category_lists()
    cats = D.DeviceCategories.from_scipy(sps.csr_array(unit), gpu)
    known, stats = D.list_category_stats(_dev(panel, gpu), cats)
    known, stats = known.cpu().numpy(), stats.cpu().numpy()
    assert known.tolist() == [0, 1, 2, 100, 37, 0]
    for q, recs in enumerate(_rows(panel)):
        items, _ = R.known(recs, N_CAT_ITEMS)
        v = unit[items]
        tri = np.sum(np.triu(v @ v.T, 1))
        k = max(len(items), 2)
        assert abs((stats[0, q] - stats[1, q]) / 2 - tri) <= 1e-10 * k * (k - 1) / 2
        assert abs(stats[1, q] - np.sum(v * v)) <= 4 * (len(items) + C) * U * max(len(items), 1)


# ---- gather mean -----------------------------------------------------------------------------


def test_gather_mean_counts_unknown_items_in_the_length(gpu):
    from lkpy_amd import _device as D

    rng = np.random.default_rng(9)
    table = rng.random(N_CAT_ITEMS)
    panel = _category_lists()
    for cutoff in (0, 50, 1):
        sums, lens = D.list_gather_mean(_dev(panel, gpu), _dev(table, gpu), cutoff)
        sums, lens = sums.cpu().numpy(), lens.cpu().numpy()
        rows = [R.truncate(r, cutoff or None) for r in _rows(panel)]
        assert lens.tolist() == [len(r) for r in rows]
        assert lens[5] == (3 if cutoff != 1 else 1) and sums[5] == 0.0  # unknown: counted, add 0
        for q, r in enumerate(rows):
            if len(r):
                want = R.mean_pop_rank(r, table)
                assert abs(sums[q] / lens[q] - want) <= len(r) * U, (cutoff, q)
    # in rank order, bit for bit
    seq = 0.0
    for i in _rows(panel)[3]:
        seq += table[i]
    sums, _ = D.list_gather_mean(_dev(panel, gpu), _dev(table, gpu), 0)
    assert sums.cpu().numpy()[3] == seq


# ---- pair statistics -------------------------------------------------------------------------


def _pair_cases(n):
    rng = np.random.default_rng(1000 + n)
    pool = rng.permutation(20000).astype(np.int32)
    base = pool[:n + 40]
    long_a = pool[100:5100].copy()
    promoted = long_a[-1]
    b_promoted = np.concatenate([long_a[:max(n - 1, 0)], [promoted]]).astype(np.int32)
    shuffled = rng.permutation(base[:n + 5])
    return [
        (base[:max(n // 2, 1)], shuffled),                 # a shorter than n
        (rng.permutation(base), base[:max(n // 3, 1)]),    # b shorter than n
        (np.zeros(0, np.int32), base[:n]),                 # a empty
        (long_a, b_promoted),                              # 5000 entries, the promoted item last
        (base, base.copy()),                               # identical
        (base, pool[6000:6000 + n + 7]),                   # disjoint
        (rng.permutation(base), rng.permutation(base)),    # the general case
        (base[:n], np.zeros(0, np.int32)),                 # b empty
    ]


@pytest.mark.parametrize("n", [1, 10, 64, 65, 1024])
def test_pair_stats_bit_identical(gpu, n):
    from lkpy_amd import _device as D

    cases = _pair_cases(n)
    weights = R.geometric_weight(np.arange(1, n + 1))
    a_ptr = np.cumsum([0] + [len(a) for a, _ in cases]).astype(np.int64)
    b_ptr = np.cumsum([0] + [len(b) for _, b in cases]).astype(np.int64)
    rbo, lip, flag = D.list_pair_stats(
        _dev(a_ptr, gpu), _dev(np.concatenate([a for a, _ in cases]).astype(np.int32), gpu),
        _dev(b_ptr, gpu), _dev(np.concatenate([b for _, b in cases]).astype(np.int32), gpu),
        n, _dev(weights, gpu))
    rbo, lip, flag = rbo.cpu().numpy(), lip.cpu().numpy(), flag.cpu().numpy()
    for q, (a, b) in enumerate(cases):
        want, _total = R.rbo_sum(a, b, weights)
        assert _bits(rbo[q]) == _bits(want), (n, q)
        want_lip = R.lip(a, b, n)
        assert flag[q] == (1 if len(a) == 0 else 0)
        if len(a):
            assert lip[q] == want_lip, (n, q)
    assert lip[3] == 4999 - n and rbo[5] == 0.0


def test_reranking_functions_and_missing_reference(gpu):
    from lkpy_amd import reranking_metrics as RM
    from lkpy_amd.data import ItemList, ItemListCollection
    from lkpy_amd.metrics import LogRankWeight

    rng = np.random.default_rng(12)
    ids = rng.permutation(500)[:60] + 7000
    a = ItemList(item_ids=ids, ordered=True)
    b = ItemList(item_ids=rng.permutation(ids)[:25], ordered=True)
    empty = ItemList(item_ids=np.zeros(0, np.int64), ordered=True)
    for n in (10, 40):
        assert RM.rank_biased_overlap(a, b, n=n) == R.rbo(ids, b.ids(), n)
        assert RM.least_item_promoted(a, b, n=n) == R.lip(ids, b.ids(), n)
    assert RM.rank_biased_overlap(a, a) == R.rbo(ids, ids) and RM.least_item_promoted(a, a) == 0
    assert math.isnan(RM.least_item_promoted(empty, b)) and RM.rank_biased_overlap(empty, b) == 0
    assert RM.rank_biased_overlap(a, b, weight=LogRankWeight(), n=7) == \
        R.rbo(ids, b.ids(), 7, lambda r: np.log(2) / np.log(np.maximum(r, 2)))
    ref = ItemListCollection.from_dict({1: a, 2: b}, key=("user_id",))
    rer = ItemListCollection.from_dict({(1, 0): b, (2, 0): b, (3, 0): a, (1, 1): a},
                                       key=("user_id", "sample"))
    s = RM.rank_biased_overlap_collection(ref, rer)
    p = RM.least_item_promoted_collection(ref, rer)
    assert s.index.names == ["user_id", "sample"] and list(s.index) == list(p.index)
    assert s[(1, 0)] == R.rbo(ids, b.ids()) and s[(2, 0)] == 1.0 and s[(1, 1)] == 1.0
    assert math.isnan(s[(3, 0)]) and math.isnan(p[(3, 0)])
    assert p[(1, 0)] == R.lip(ids, b.ids()) and p[(2, 0)] == 0


# ---- end to end ------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def synth_run(gpu):
    "ml-latest-small sized synthetic data, an ImplicitMF pipeline, a test split of 120 users"
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.splitting import SampleFrac, sample_users
    from lkpy_amd.training import TrainingOptions

    rng = np.random.default_rng(2026)
    n_users, n_items = 610, 9724
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.9
    pop /= pop.sum()
    us, its = [], []
    for u in range(n_users):
        deg = int(min(20 + rng.pareto(1.2) * 60, 1500))
        its.append(rng.choice(n_items, deg, replace=False, p=pop))
        us.append(np.full(deg, u))
    ds = Dataset.from_arrays(np.concatenate(us) + 1, np.concatenate(its) + 10,
                             all_item_ids=np.arange(n_items) + 10)
    genres = (rng.random((n_items, 20)) < 0.12).astype(np.float64)
    ds.item_attrs["genre"] = sps.csr_array(genres)
    split = sample_users(ds, 120, SampleFrac(0.2, rng=7), rng=7)
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=16, epochs=2))
    pipe.train(split.train, TrainingOptions(rng=7))
    return ds, genres, split, pipe


def test_end_to_end_three_routes_one_frame(gpu, synth_run):
    import torch

    from lkpy_amd import batch
    from lkpy_amd import metrics as M

    ds, genres, split, pipe = synth_run
    train = split.train
    users = M.pack_collection(split.test).key_columns()["user_id"]
    recs = batch.recommend(pipe, users, 20)

    def analysis():
        return M.RunAnalysis(
            M.NDCG(10), M.RBP(), M.Hit(5), M.Recall(),
            M.ListGini(items=train), M.ExposureGini(10, items=train.items),
            M.ILS(train, "genre", 10), M.Entropy(train, "genre"),
            M.RankBiasedEntropy(categories=genres, items=train.items, attribute="dense", n=15),
            M.MeanPopRank(train), M.MeanPopRank(train, n=5, count="interactions"))

    ra = analysis()
    res = ra.measure(recs, split.test)
    frame, summary = res.list_metrics(fill_missing=False), res.global_metrics()
    assert "ListGini" not in frame and "ExposureGini@10" not in frame
    assert 0 < summary["ListGini"] < 1 and 0 < summary["ExposureGini@10"] < 1

    nums = recs._lists.nums
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    d_idx, _sc = scorer.recommend_batch(lookup.batch(users), 20, device_output=True)
    assert isinstance(d_idx, torch.Tensor) and d_idx.is_cuda
    for panel in (nums, d_idx):
        mc = ra.collector.empty_copy()
        mc.add_array_measurements(users, panel, split.test, vocabulary=scorer.items)
        f2, s2 = mc.list_metrics(), mc.summary_metrics()
        assert list(f2.columns) == list(frame.columns)
        for c in frame.columns:
            assert np.array_equal(_bits(f2[c]), _bits(frame[c])), c
        assert set(s2) == set(summary.index)
        for k in s2:
            assert _bits(s2[k]) == _bits(summary[k]), k

    # the values themselves, against the restatement
    unit, dist = R.normalize_rows(genres, "unit"), R.normalize_rows(genres, "distribution")
    table = R.pop_table(np.bincount(train._cols, minlength=len(train.items)))  # (no repeats)
    rows = _rows(nums)
    for lbl, f, tol in (
            ("ILS(genre)@10", lambda r: R.ils(r, unit, 10), 1e-10),
            ("Entropy(genre)", lambda r: R.entropy(r, dist), 1e-10 * math.log2(21)),
            ("RBEntropy(dense)@15", lambda r: R.entropy(r, dist, 15, R.geometric_weight),
             1e-10 * math.log2(21)),
            ("MeanPopRank", lambda r: R.mean_pop_rank(r, table), 20 * U),
            ("MeanPopRank@5", lambda r: R.mean_pop_rank(r, table, 5), 5 * U)):
        want = np.array([f(r) for r in rows])
        assert np.all(np.abs(frame[lbl].to_numpy() - want) <= tol), lbl
    assert _bits(summary["ListGini"]) == \
        _bits(R.gini_of_totals(R.exposure_totals(rows, len(train.items))))
    assert _bits(summary["ExposureGini@10"]) == _bits(R.gini_of_totals(
        R.exposure_totals(rows, len(train.items), 10, R.geometric_weight)))


def test_samples_against_the_deterministic_lists(gpu, synth_run):
    from lkpy_amd import batch
    from lkpy_amd import metrics as M
    from lkpy_amd import reranking_metrics as RM
    from lkpy_amd.stochastic import StochasticTopNRanker

    ds, genres, split, pipe = synth_run
    users = M.pack_collection(split.test).key_columns()["user_id"][:40]
    base = batch.recommend(pipe, users, 50)
    pipe.replace_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                           query="history-lookup")
    many = batch.recommend_samples(pipe, users, 10, 4)
    assert many.key_fields == ("user_id", "sample") and len(many) == 160
    rbo = RM.rank_biased_overlap_collection(base, many)
    lip = RM.least_item_promoted_collection(base, many)
    assert len(rbo) == 160 and rbo.index.names == ["user_id", "sample"]
    for (u, s), il in many:
        ref = base.lookup(u)
        assert _bits(rbo[(u, s)]) == _bits(RM.rank_biased_overlap(ref, il)), (u, s)
        assert _bits(lip[(u, s)]) == _bits(RM.least_item_promoted(ref, il)), (u, s)
        assert _bits(rbo[(u, s)]) == _bits(R.rbo(ref.ids(), il.ids()))
    assert 0 < rbo.mean() < 1
