"""
The FunkSVD trainer on the device (csrc/funksvd.hip, ``lkpy_amd._device.funksvd_fit``) and
``lkpy_amd.funksvd.FunkSVDScorer``.

Bars.  Embeddings: ``np.array_equal`` on the uint32 views against the sequential restatement
(``tests/funksvd_restatement.py``: the reference's arithmetic in Python floats).  The squared
error of an epoch: ``n 2^-52`` relative -- the device's and the restatement's are float64 sums of
the same n non-negative terms in two orders, and a sum of n non-negative terms is within
``(n - 1) 2^-53`` relative of the exact sum in any order.  ``__call__``: ``(k + 3) 2^-23 sum
|terms|`` against the float64 formula, k + 3 float32 terms in one sum.  The batch routes: the bits
of ``pipe.run``.  The recorded predictions: the reference's own 0.01.
"""
import pickle
import time
from pathlib import Path

import numpy as np
import pytest

import funksvd_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
LR, REG = 0.001, 0.015


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_fit(got, want):
    assert got[0].dtype == np.float32 and got[0].shape == want[0].shape
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


def _sse_close(stats, got_rmse, want_sse, n):
    "the kernel's squared errors (``stats['sse']``) and the RMSE made of them"
    got = stats["sse"]
    assert got.shape == want_sse.shape and got.dtype == np.float64
    assert np.all(np.abs(got - want_sse) <= n * 2.0 ** -52 * want_sse), (got, want_sse)
    assert np.array_equal(got_rmse, np.sqrt(got / n))


def _rmse_close(got_rmse, want_sse, n):
    """a component's ``training_rmse_``: the square root halves the relative distance of the two
    sums ((n - 1) 2^-52) and the division and the root round once each -- within n 2^-52"""
    want = np.sqrt(want_sse / n)
    assert got_rmse.shape == want.shape
    assert np.all(np.abs(got_rmse - want) <= n * 2.0 ** -52 * want), (got_rmse, want)


# ---- the plan ---------------------------------------------------------------------------------
def test_plan_matches_the_restatement(gpu):
    from lkpy_amd import _device as D

    users, items, _, _ = R.case_cross(300, 200, seed=5)
    got = D.funksvd_plan(users, items, 300, 200)
    level = R.levels(users, items, 300, 200)
    order, ptr, run_end = R.plan(level)
    assert np.array_equal(got.level, level)
    assert np.array_equal(got.order, order) and np.array_equal(got.level_ptr, ptr)
    assert np.array_equal(got.run_end, run_end)


# ---- the kernel -------------------------------------------------------------------------------
CROSS = {"none": None, "clamped": (1.0, 4.5)}


@pytest.fixture(scope="module")
def cross():
    "300 x 200, about 6 000 ratings, k = 3, 4 epochs: the case and its restated fits"
    case = R.case_cross(300, 200, seed=5)
    fits = {name: R.train(*case, 300, 200, 3, 4, LR, REG, rr) for name, rr in CROSS.items()}
    assert fits["none"][3] == 0 and fits["clamped"][3] > 0  # the clamp acts in the second
    assert not np.array_equal(fits["none"][0], fits["clamped"][0])
    return case, fits


@pytest.mark.parametrize("global_columns", [False, True])
@pytest.mark.parametrize("name", list(CROSS))
def test_cross_case(gpu, cross, name, global_columns):
    from lkpy_amd import _device as D

    case, fits = cross
    rr = CROSS[name] or (-np.inf, np.inf)
    before = case[3].copy()
    stats = {}
    got = D.funksvd_fit(*case, 300, 200, 3, 4, LR, REG, *rr, global_columns=global_columns,
                        stats=stats)
    assert np.array_equal(case[3], before)  # the caller's estimates are not touched
    _same_fit(got, fits[name])
    assert got[2].shape == (3, 4)
    _sse_close(stats, got[2], fits[name][2], len(case[0]))


def test_epochs_split_over_launches(gpu, cross):
    "1 + 1 + 1 + 1 epochs against one launch: the same bits, the same squared errors"
    from lkpy_amd import _device as D

    case, fits = cross
    n = len(case[0])
    for global_columns in (False, True):
        stats_one, stats_four = {}, {}
        one = D.funksvd_fit(*case, 300, 200, 3, 4, LR, REG, 1.0, 4.5, stats=stats_one,
                            global_columns=global_columns)
        four = D.funksvd_fit(*case, 300, 200, 3, 4, LR, REG, 1.0, 4.5, step_budget=n,
                             stats=stats_four, global_columns=global_columns)
        assert stats_one["epochs_per_launch"] == 4 and stats_four["epochs_per_launch"] == 1
        _same_fit(four, one)
        _same_fit(four, fits["clamped"])
        assert np.array_equal(one[2], four[2])
    # a budget below one epoch still runs whole epochs
    tiny = D.funksvd_fit(*case, 300, 200, 3, 4, LR, REG, 1.0, 4.5, step_budget=1)
    _same_fit(tiny, one)


@pytest.fixture(scope="module")
def matchings():
    case = R.case_matchings()
    return case, R.train(*case[:4], 1025, 1025, 2, 2, LR, REG, (1.0, 4.5))


@pytest.mark.parametrize("global_columns", [False, True])
def test_stacked_matchings(gpu, matchings, global_columns):
    """level widths 65 64 63 1 1 70 1024 1025 2 64: the wave seam, the stride seam, narrow runs
    entered and left -- the schedule is given, one matching a level"""
    from lkpy_amd import _device as D

    (users, items, ratings, est, level), want = matchings
    assert want[3] > 0
    plan = D.funksvd_plan_of_levels(level)
    assert list(np.diff(plan.level_ptr)) == R.MATCHING_WIDTHS
    assert list(plan.run_end) == [0, 5, 5, 5, 5, 5, 6, 7, 10, 10]
    stats = {}
    got = D.funksvd_fit(users, items, ratings, est, 1025, 1025, 2, 2, LR, REG, 1.0, 4.5,
                        plan=plan, global_columns=global_columns, stats=stats)
    _same_fit(got, want)
    _sse_close(stats, got[2], want[2], len(users))
    # the shallowest schedule of the same samples: other levels, the same bits
    own = D.funksvd_fit(users, items, ratings, est, 1025, 1025, 2, 2, LR, REG, 1.0, 4.5,
                        global_columns=global_columns)
    _same_fit(own, want)


def test_a_schedule_with_a_repeat_is_refused(gpu, matchings):
    from lkpy_amd import _device as D

    (users, items, ratings, est, level), _ = matchings
    bad = level.copy()
    bad[65:] = np.maximum(bad[65:] - 1, 0)  # the second matching joins the first
    with pytest.raises(ValueError, match="repeats inside a level"):
        D.funksvd_fit(users, items, ratings, est, 1025, 1025, 2, 2, LR, REG,
                      plan=D.funksvd_plan_of_levels(bad))


def test_columns_beyond_the_lds_budget(gpu):
    "40 000 users of one rating each: the columns do not fit LDS, whatever the hook says"
    from lkpy_amd import _device as D

    case = R.case_singletons()
    assert (40000 + 50) * 4 > D.funksvd_lds_column_bytes()
    want = R.train(*case, 40000, 50, 1, 2, LR, REG, (1.0, 4.5))
    assert want[3] > 0
    stats = {}
    got = D.funksvd_fit(*case, 40000, 50, 1, 2, LR, REG, 1.0, 4.5, stats=stats)
    _same_fit(got, want)
    _sse_close(stats, got[2], want[2], 40000)


def test_fit_preconditions(gpu):
    from lkpy_amd import _device as D

    u = np.array([0, 1, 5], np.int32)
    i = np.array([0, 1, 1], np.int32)
    r = np.ones(3, np.float32)
    with pytest.raises(ValueError, match="outside"):
        D.funksvd_fit(u, i, r, r, 3, 2, 1, 1, LR, REG)
    with pytest.raises(ValueError, match="positive"):
        D.funksvd_fit(u, i, r, r, 6, 2, 0, 1, LR, REG)
    with pytest.raises(ValueError, match="one length"):
        D.funksvd_fit(u, i[:2], r, r, 6, 2, 1, 1, LR, REG)


# ---- the component on the reference's 4-rating data -----------------------------------------
def _simple_ds():
    import pandas as pd

    from lkpy_amd.data import from_interactions_df

    df = pd.DataFrame({"item": [1, 1, 2, 3], "user": [10, 12, 10, 13],
                       "rating": [4.0, 3.0, 5.0, 2.0]})
    return df, from_interactions_df(df)


def _restate(ds, sc, shuf):
    "the restatement of ``sc``'s fit of ``ds`` from the sample order ``shuf`` and a host bias fit"
    from lkpy_amd.basic import BiasModel

    cfg = sc.config
    bias = BiasModel.learn(ds, cfg.damping)
    users, items = ds._rows[shuf], ds._cols[shuf]
    ratings = ds._attrs["rating"][shuf]
    est = R.initial_estimates(users, items, bias.global_bias, bias.item_biases, bias.user_biases)
    return R.train(users, items, ratings, est, ds.user_count, ds.item_count, cfg.embedding_size,
                   cfg.epochs, cfg.learning_rate, cfg.regularization, cfg.range)


@pytest.mark.parametrize("rng_range", [None, (1, 5)])
def test_simple_ds(gpu, rng_range):
    "tests/funksvd/test_funksvd.py of the reference: its assertions, and the restatement's bits"
    from lkpy_amd.data import ItemList
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.training import TrainingOptions

    df, ds = _simple_ds()
    algo = FunkSVDScorer(features=20, epochs=20, range=rng_range)
    assert algo.config.embedding_size == 20
    algo.train(ds, TrainingOptions(rng=42))
    assert algo.bias.global_bias == pytest.approx(df.rating.mean())
    assert algo.item_embeddings.shape == (3, 20) and algo.user_embeddings.shape == (3, 20)
    assert algo.training_rmse_.shape == (20, 20)
    shuf = np.arange(4)
    np.random.default_rng(42).shuffle(shuf)
    want = _restate(ds, algo, shuf)
    _same_fit((algo.user_embeddings, algo.item_embeddings), want)
    _rmse_close(algo.training_rmse_, want[2], 4)

    preds = algo(query=10, items=ItemList([3]))
    assert len(preds) == 1 and preds.ids()[0] == 3
    lo = 0 if rng_range is None else 1
    assert lo <= preds.scores()[0] <= 5
    bad_item = algo(10, ItemList([4]))
    assert len(bad_item) == 1 and bad_item.ids()[0] == 4 and np.isnan(bad_item.scores()[0])
    bad_user = algo(query=50, items=ItemList([3]))
    assert len(bad_user) == 1 and bad_user.ids()[0] == 3 and np.isnan(bad_user.scores()[0])

    # the order hook replaces the shuffle; the global-column hook changes no bit
    hooked = FunkSVDScorer(features=20, epochs=20, range=rng_range)
    hooked._order, hooked._global_columns = shuf, True
    hooked.train(ds, TrainingOptions(rng=7))
    _same_fit((hooked.user_embeddings, hooked.item_embeddings), want)


# ---- the component on ml-latest-small --------------------------------------------------------
@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def test_ml_slice_matches_the_restatement(gpu, ml):
    "5 000 ratings of ml-latest-small, k = 2, 3 epochs, seeded: the reference's order and bits"
    from lkpy_amd.data import Dataset
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.training import TrainingOptions

    take = np.sort(np.random.default_rng(3).choice(len(ml._rows), 5000, replace=False))
    ds = Dataset.from_arrays(ml.users.ids()[ml._rows[take]], ml.items.ids()[ml._cols[take]],
                             ml._attrs["rating"][take])
    sc = FunkSVDScorer(features=2, epochs=3, range=(0.5, 4.5))
    sc.train(ds, TrainingOptions(rng=11))
    shuf = np.arange(5000)
    np.random.default_rng(11).shuffle(shuf)
    want = _restate(ds, sc, shuf)
    assert want[3] > 0
    _same_fit((sc.user_embeddings, sc.item_embeddings), want)
    _rmse_close(sc.training_rmse_, want[2], 5000)


@pytest.fixture(scope="module")
def trained(ml, gpu):
    "the golden pipeline (15 features, 20 epochs) trained on ml-latest-small"
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "funksvd.toml")
    pipe.train(ml, TrainingOptions(rng=21))
    return pipe


def test_component_state_pickle_and_retrain(ml, trained):
    from lkpy_amd.data import ItemList
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.training import TrainingOptions

    sc = trained.node("scorer").component
    assert isinstance(sc, FunkSVDScorer) and sc.is_trained()
    assert sc.users is ml.users and sc.items is ml.items
    assert sc.user_embeddings.shape == (ml.user_count, 15)
    assert sc.item_embeddings.shape == (ml.item_count, 15)
    assert sc.user_embeddings.dtype == np.float32 and sc.item_embeddings.dtype == np.float32
    assert np.isfinite(sc.user_embeddings).all() and np.isfinite(sc.item_embeddings).all()
    assert sc.training_rmse_.shape == (15, 20)
    assert (np.diff(sc.training_rmse_[0]) < 0).all() and 0.7 < sc.training_rmse_[-1, -1] < 1.0
    assert sc.bias.global_bias == pytest.approx(float(np.mean(ml._attrs["rating"])))
    il = ItemList(item_ids=np.concatenate([ml.items.ids()[:300], [-5]]))
    uid = ml.users.ids()[9].item()
    got = sc(uid, il).scores()
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__
    assert np.array_equal(_bits(sc2.user_embeddings), _bits(sc.user_embeddings))
    assert np.array_equal(_bits(sc2.item_embeddings), _bits(sc.item_embeddings))
    assert np.array_equal(sc2.training_rmse_, sc.training_rmse_)
    assert np.array_equal(_bits(sc2(uid, il).scores()), _bits(got))
    before = sc.user_embeddings
    sc.train(ml, TrainingOptions(rng=9, retrain=False))
    assert sc.user_embeddings is before


def test_seeded_fits_repeat(gpu, ml):
    from lkpy_amd.data import Dataset
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.training import TrainingOptions

    take = np.arange(0, len(ml._rows), 20)
    ds = Dataset.from_arrays(ml._rows[take], ml._cols[take], ml._attrs["rating"][take])
    fits = []
    for seed in (7, 7, 8):
        sc = FunkSVDScorer(features=2, epochs=2)
        sc.train(ds, TrainingOptions(rng=seed))
        fits.append(sc)
    assert np.array_equal(_bits(fits[0].item_embeddings), _bits(fits[1].item_embeddings))
    assert np.array_equal(fits[0].training_rmse_, fits[1].training_rmse_)  # a fixed-order sum
    assert not np.array_equal(fits[0].item_embeddings, fits[2].item_embeddings)


def test_call_against_the_host_formula(ml, trained):
    from lkpy_amd.data import ItemList

    sc = trained.node("scorer").component
    k = sc.config.embedding_size
    items = np.arange(40, 140)
    il = ItemList(item_ids=np.concatenate([ml.items.ids()[items], [-5]]))
    for u in (0, 17, 300):
        got = sc(ml.users.ids()[u].item(), il).scores()
        assert got.dtype == np.float32 and np.isnan(got[-1])
        p = sc.user_embeddings[u].astype(np.float64)
        q = sc.item_embeddings[items].astype(np.float64)
        g, bi, bu = sc.bias.global_bias, sc.bias.item_biases[items], sc.bias.user_biases[u]
        want = R.score(sc.user_embeddings[u], sc.item_embeddings[items], g, bi, bu)
        size = np.abs(q) @ np.abs(p) + abs(g) + np.abs(bi) + abs(bu)
        assert (np.abs(got[:-1] - want) <= (k + 3) * 2.0 ** -23 * size).all()
    assert np.isnan(sc(-777, il).scores()).all() and np.isnan(sc(None, il).scores()).all()


def _same_lists(got, want, what):
    assert np.array_equal(got.ids(), want.ids()), what
    assert np.array_equal(_bits(got.scores()), _bits(want.scores())), what


def test_batch_routes_are_the_pipeline_per_query(ml, trained):
    """score_batch, batch.predict, batch.score, batch.recommend and recommend(candidates=)
    against ``pipe.run`` query by query, bit for bit -- among them a query whose rated history
    changes its user bias"""
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList, RecQuery

    pipe = trained
    sc = pipe.node("scorer").component
    ids, uids = ml.items.ids(), ml.users.ids()
    users = [uids[3 * i].item() for i in range(24)]
    pairs = {u: ItemList(item_ids=np.concatenate([ids[7 * n:7 * n + 12 + n], [-5]]))
             for n, u in enumerate(users)}

    # score_batch, with a query that carries its own ratings and an unknown user
    hist = ItemList(item_ids=ids[[1, 2, 3]], rating=np.array([5.0, 5.0, 4.5]))
    rated = RecQuery(user_id=users[0], user_items=hist)
    queries = [rated, *users[1:], -777]
    lists = [*pairs.values(), pairs[users[0]]]
    for q, il, got in zip(queries, lists, sc.score_batch(queries, lists)):
        _same_lists(got, sc(q, il), q)
    plain = sc(users[0], pairs[users[0]]).scores()
    moved = sc(rated, pairs[users[0]]).scores()
    _, want_ub = sc.bias.compute_for_items(pairs[users[0]], users[0], hist)
    un = ml.users.number(users[0])
    shift = float(want_ub) - float(sc.bias.user_biases[un])
    assert abs(shift) > 0.05
    assert np.allclose(moved[:-1] - plain[:-1], shift, rtol=0, atol=1e-5)

    preds = batch.predict(pipe, pairs)
    scored = batch.score(pipe, pairs)
    for u, il in pairs.items():
        _same_lists(preds.lookup(u), pipe.run("rating-predictor", query=u, items=il), u)
        _same_lists(scored.lookup(u), pipe.run("scorer", query=u, items=il), u)
        assert np.isfinite(scored.lookup(u).scores()[:-1]).all()

    recs = batch.recommend(pipe, np.asarray(users), 10)
    for u in users:
        got = recs.lookup(u)
        _same_lists(got, pipe.run("recommender", query=u, n=10), u)
        un = ml.users.number(u)
        assert len(got) == 10 and not np.isin(
            got.numbers(vocabulary=ml.items), ml._cols[ml._indptr[un]:ml._indptr[un + 1]]).any()

    cands = {u: ids[11 * n:11 * n + 60] for n, u in enumerate(users)}
    ranked = batch.recommend(pipe, None, 10, candidates=cands)
    for u in users:
        _same_lists(ranked.lookup(u),
                    pipe.run("recommender", query=u, items=ItemList(item_ids=cands[u]), n=10), u)


def test_recorded_predictions(gpu, ml):
    """the reference's ``test_fsvd_known_preds``: ml-latest-small, 15 features, 125 epochs, every
    one of its 2 000 recorded predictions within its own 0.01"""
    import pandas as pd

    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.pipeline import predict_pipeline
    from lkpy_amd.training import TrainingOptions

    known = pd.read_csv(GOLDEN / "funksvd-preds.csv")
    algo = FunkSVDScorer(features=15, epochs=125, lrate=0.001)
    pipe = predict_pipeline(algo, fallback=False)
    t0 = time.perf_counter()
    pipe.train(ml, TrainingOptions(rng=42))  # (the reference's test is unseeded; any seed serves)
    print(f"recorded predictions: trained 15 x 125 epochs in {time.perf_counter() - t0:.2f} s, "
          f"final training RMSE {algo.training_rmse_[-1, -1]:.4f}")
    pairs = {u: ItemList(item_ids=g.item_id.to_numpy()) for u, g in known.groupby("user_id")}
    preds = batch.predict(pipe, pairs)
    worst = 0.0
    for u, g in known.groupby("user_id"):
        got = preds.lookup(u)
        assert np.array_equal(got.ids(), g.item_id.to_numpy())
        score, expected = got.scores().astype(np.float64), g.prediction.to_numpy()
        assert not (np.isnan(score) & ~np.isnan(expected)).any()
        err = np.abs(expected - score)[~np.isnan(expected)]
        worst = max(worst, float(err.max()))
    print(f"recorded predictions: worst error {worst:.5f} (bar 0.01)")
    assert worst < 0.01
