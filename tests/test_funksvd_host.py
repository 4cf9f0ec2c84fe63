"""
FunkSVD's host side: the level schedule (``tests/funksvd_restatement.py`` and the native
``lk_funksvd_plan_*``, which need no device), that walking the samples level by level gives the
bits of the sequential walk, the configuration and the pipeline file.  No GPU.
"""
from pathlib import Path

import numpy as np
import pytest

import funksvd_restatement as R

GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def case():
    "300 x 200, about 6 000 shuffled ratings: a full user, a full item, two duplicated pairs"
    return R.case_cross(300, 200, seed=5)


@pytest.fixture(scope="module")
def level(case):
    users, items, _, _ = case
    return R.levels(users, items, 300, 200)


def test_level_schedule_properties(case, level):
    users, items, _, _ = case
    order, ptr, run_end = R.plan(level)
    depth = len(ptr) - 1
    assert ptr[0] == 0 and ptr[-1] == len(users) and (np.diff(ptr) > 0).all()
    # within one level no user and no item repeats
    for ent in (users, items):
        for l in range(depth):
            seg = ent[order[ptr[l]:ptr[l + 1]]]
            assert len(np.unique(seg)) == len(seg), l
    # ascending sample position inside a level; every user's and item's samples keep their order
    for l in range(depth):
        assert (np.diff(order[ptr[l]:ptr[l + 1]]) > 0).all()
    for ent, count in ((users, 300), (items, 200)):
        walked = ent[order]
        for x in range(count):
            assert np.array_equal(order[walked == x], np.flatnonzero(ent == x))
    # no exact order is shallower than the busiest chain
    degree = max(np.bincount(users).max(), np.bincount(items).max())
    assert degree == 300 and depth >= degree
    # the narrow-run marks: runs of narrow levels, as long as the stage allows
    width = np.diff(ptr)
    l, runs, longest, capped = 0, 0, 0, 0
    while l < depth:
        e = run_end[l]
        if width[l] > R.NARROW:
            assert e == l
            l += 1
            continue
        assert e > l and (run_end[l:e] == e).all() and (width[l:e] <= R.NARROW).all()
        assert ptr[e] - ptr[l] <= R.STAGE
        assert e == depth or width[e] > R.NARROW or ptr[e + 1] - ptr[l] > R.STAGE
        capped += e < depth and width[e] <= R.NARROW
        l, runs, longest = e, runs + 1, max(longest, e - l)
    # the case has a run cut by the stage and one of more levels than a wave has lanes
    assert runs > 1 and (width > R.NARROW).any() and capped > 0 and longest > 64


@pytest.mark.parametrize("rng_range", [None, (1.0, 4.5)])
def test_level_order_equals_sequential_order(case, level, rng_range):
    users, items, ratings, est = case
    order, _, _ = R.plan(level)
    assert not np.array_equal(order, np.arange(len(order)))
    seq = R.train(users, items, ratings, est, 300, 200, 3, 4, 0.001, 0.015, rng_range)
    lev = R.train(users, items, ratings, est, 300, 200, 3, 4, 0.001, 0.015, rng_range, order)
    assert np.array_equal(seq[0].view(np.uint32), lev[0].view(np.uint32))
    assert np.array_equal(seq[1].view(np.uint32), lev[1].view(np.uint32))
    assert not np.array_equal(seq[0], np.full_like(seq[0], 0.1))
    # the clamp acts with the range, and only then
    assert (seq[3] > 0) == (rng_range is not None) and seq[3] == lev[3]
    # the squared error is the same sum in another order
    assert np.allclose(seq[2], lev[2], rtol=len(users) * 2.0 ** -52, atol=0)


def test_native_plan_matches_the_restatement(case, level):
    from lkpy_amd import _device as D

    users, items, _, _ = case
    got = D.funksvd_plan(users, items, 300, 200)
    order, ptr, run_end = R.plan(level)
    assert np.array_equal(got.level, level) and got.depth == len(ptr) - 1
    assert np.array_equal(got.order, order) and got.order.dtype == np.int64
    assert np.array_equal(got.level_ptr, ptr) and got.level_ptr.dtype == np.int64
    assert np.array_equal(got.run_end, run_end)
    again = D.funksvd_plan_of_levels(level)
    assert np.array_equal(again.order, order) and np.array_equal(again.run_end, run_end)
    empty = D.funksvd_plan(np.zeros(0, np.int32), np.zeros(0, np.int32), 3, 4)
    assert empty.depth == 0 and len(empty.order) == 0 and list(empty.level_ptr) == [0]
    with pytest.raises(ValueError, match="outside"):
        D.funksvd_plan(np.array([0, 3], np.int32), np.array([0, 1], np.int32), 3, 4)
    with pytest.raises(ValueError, match="outside"):
        D.funksvd_plan(np.array([0, 1], np.int32), np.array([0, -1], np.int32), 3, 4)


def test_native_plan_on_ml_small():
    "the depth is the busiest user's rating count: no exact order has fewer levels"
    from lkpy_amd import _device as D
    from lkpy_amd.data import load_movielens_npz

    ds = load_movielens_npz(GOLDEN / "ml_small.npz")
    shuf = np.arange(len(ds._rows))
    np.random.default_rng(1).shuffle(shuf)
    users, items = ds._rows[shuf], ds._cols[shuf]
    plan = D.funksvd_plan(users, items, ds.user_count, ds.item_count)
    assert plan.depth == np.bincount(users).max() == 2391
    assert np.array_equal(plan.level, R.levels(users, items, ds.user_count, ds.item_count))


def test_stacked_matchings_case():
    users, items, _, _, level = R.case_matchings()
    assert list(np.bincount(level)) == R.MATCHING_WIDTHS
    order, ptr, run_end = R.plan(level)
    assert np.array_equal(order, np.arange(len(users)))
    for l in range(len(ptr) - 1):
        for ent in (users, items):
            seg = ent[ptr[l]:ptr[l + 1]]
            assert len(np.unique(seg)) == len(seg)
    # widths 65 64 63 1 1 70 1024 1025 2 64: two narrow runs, entered and left
    assert list(run_end) == [0, 5, 5, 5, 5, 5, 6, 7, 10, 10]


def test_config():
    from lkpy_amd.funksvd import FunkSVDConfig, FunkSVDScorer

    cfg = FunkSVDConfig()
    assert (cfg.embedding_size, cfg.epochs, cfg.learning_rate, cfg.regularization, cfg.damping,
            cfg.range) == (64, 100, 0.001, 0.015, 5.0, None)
    assert FunkSVDConfig(features=12).embedding_size == 12
    assert FunkSVDConfig(embedding_size=7).embedding_size == 7
    assert FunkSVDConfig(embedding_size_exp=4).embedding_size == 16
    assert FunkSVDConfig(range=[1, 5]).range == (1.0, 5.0)
    # the reference's own test passes ``lrate=``: an unknown key is ignored
    sc = FunkSVDScorer(features=15, epochs=125, lrate=0.001)
    assert sc.config.embedding_size == 15 and sc.config.epochs == 125
    assert sc.config.learning_rate == 0.001 and not sc.is_trained()
    assert "lrate" not in sc.dump_config()


def test_class_path_and_pipeline_file():
    from lkpy_amd.funksvd import FunkSVDScorer
    from lkpy_amd.pipeline import Pipeline, import_path_string

    assert import_path_string("lenskit.funksvd.FunkSVDScorer") is FunkSVDScorer
    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "funksvd.toml")
    sc = pipe.node("scorer").component
    assert isinstance(sc, FunkSVDScorer)
    assert sc.config.embedding_size == 15 and sc.config.epochs == 20


def test_recorded_predictions_file():
    import pandas as pd

    known = pd.read_csv(GOLDEN / "funksvd-preds.csv")
    assert list(known.columns) == ["user_id", "item_id", "prediction"] and len(known) == 2000
