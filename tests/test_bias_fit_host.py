"""The bias fit's order, proven on the host: the plain-loop restatement of what csrc/bias.hip
computes (``tests/bias_restatement.py``: per-bin chains over the CSR and a stable transpose) gives
the bits of ``BiasModel.learn`` on the GPU test's matrix, and the three reassociations a kernel
might make (a ``damping + n`` count, a pairwise or a reversed bin sum) do not;
``learn(device=None)`` is the parent commit's arithmetic; and which Bias
pipelines the batch entry points take as whole batches.  No device is touched."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bias_restatement as R  # noqa: E402

THIRD = (100 / 3, 100 / 3)


@pytest.fixture(scope="module")
def ds():
    return R.matrix_dataset()


def _host(ds, damping, entities):
    from lkpy_amd.basic import BiasModel

    return BiasModel.learn(ds, damping, entities=entities)


def test_learn_without_a_device_is_the_parents_arithmetic(ds):
    for damping in R.DAMPINGS:
        for entities in R.ENTITIES:
            m = _host(ds, damping, entities)
            g, ib, ub = R.parent_learn(ds, damping, entities)
            assert m.global_bias == g and m.device_biases is None
            assert R.same_bits(m.item_biases, ib) and R.same_bits(m.user_biases, ub)
            assert (m.items is None) == ("item" not in entities)
            assert (m.users is None) == ("user" not in entities)


@pytest.mark.parametrize("damping", R.DAMPINGS, ids=str)
def test_the_kernels_order_gives_the_hosts_bits(ds, damping):
    for entities in R.ENTITIES:
        m = _host(ds, damping, entities)
        ib, ub = R.fit(ds._rows, ds._cols, ds._attrs["rating"], ds.user_count, ds.item_count,
                       m.global_bias, damping, entities)
        assert R.same_bits(ib, m.item_biases), (damping, entities)
        assert R.same_bits(ub, m.user_biases), (damping, entities)


def _differing(ds, variant):
    m = _host(ds, THIRD, ("user", "item"))
    ib, ub = R.fit(ds._rows, ds._cols, ds._attrs["rating"], ds.user_count, ds.item_count,
                   m.global_bias, THIRD, ("user", "item"), variant=variant)
    items = np.flatnonzero(ib.view(np.uint32) != m.item_biases.view(np.uint32))
    users = np.flatnonzero(ub.view(np.uint32) != m.user_biases.view(np.uint32))
    print(f"{variant}: {len(items)} item biases and {len(users)} user biases differ")
    return items.tolist(), users.tolist()


@pytest.mark.parametrize("variant", ["pairwise", "reversed"])
def test_a_reassociated_sum_has_other_bits(ds, variant):
    """The matrix tells the kernel's order from a reassociated bin sum: the GPU test would catch
    one.  Only the planted users can show it (``bias_restatement._planted``): the item pass sums
    ``r - mu``, multiples of 2^-24 whose float64 sums are exact in any order, and the float64 sum of
    an ordinary row moves by a last place at the most, which the float32 bias does not show."""
    items, users = _differing(ds, variant)
    assert items == [] and users and set(users) <= set(R.PLANTED_USERS)


def test_a_plain_count_has_other_bits(ds):
    """``damping + n`` against the chain: the two float64 counts differ by a last place, which the
    float32 bias shows where ``sum / count`` lies by a rounding midpoint.  The planted item
    (``bias_restatement._count_item_values``) is such a bin: its bias differs, and with it the
    biases of the users who rated it."""
    items, users = _differing(ds, "plain_count")
    assert items == [R.COUNT_ITEM] and users
    for keys, n_bins in ((ds._rows, ds.user_count), (ds._cols, ds.item_count)):
        counts = np.full(n_bins, 100 / 3)  # the chain is what np.add.at computes
        np.add.at(counts, keys, 1)
        assert np.array_equal(counts.view(np.uint64),
                              R.count_chains(keys, n_bins, 100 / 3).view(np.uint64))


def test_count_chain_is_not_damping_plus_n():
    "the issue's figure: for damping = 100 / 3 the two differ from a length of 223 on"
    count, first, differ = np.float64(100 / 3), None, 0
    for n in range(1, 5000):
        count = count + np.float64(1.0)
        if count != np.float64(100 / 3) + np.float64(n):
            differ += 1
            first = first or n
    assert first == 223 and differ == 2217


# ---- routing ------------------------------------------------------------------------------------
def _small(ratings=True, dtype=np.float32):
    from lkpy_amd.data import Dataset, Vocabulary

    rng = np.random.default_rng(4)
    us, its = rng.integers(0, 30, 400), rng.integers(0, 20, 400)
    attrs = {"rating": rng.uniform(0.5, 5, 400).astype(dtype)} if ratings else {}
    return Dataset(Vocabulary(np.arange(30), "user", reorder=False),
                   Vocabulary(np.arange(20), "item", reorder=False), us, its, attrs)


def _pipe(data, *, fallback=None, lookup_data=None, **config):
    "a Bias pipeline trained on the host: std:topn, or std:topn-predict with / without fallback"
    from lkpy_amd.basic import BiasScorer
    from lkpy_amd.pipeline import predict_pipeline, topn_pipeline
    from lkpy_amd.training import TrainingOptions

    scorer = BiasScorer(**config)
    pipe = topn_pipeline(scorer) if fallback is None else predict_pipeline(scorer,
                                                                           fallback=fallback)
    if data is not None:
        pipe.train(data, TrainingOptions(device="cpu"))
    if lookup_data is not None:
        pipe.node("history-lookup").component.train(lookup_data)
    return pipe


def test_routes_of_bias_pipelines():
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer

    data = _small()
    assert BiasScorer.accepts_history_batch and BiasScorer.returns_device_lists
    for fallback in (None, False, True):
        pipe = _pipe(data, fallback=fallback, damping=5.0)
        scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
        assert scorer.model.device_biases is None  # (trained on the host)
        plan = batch._candidate_route(pipe)
        assert plan is not None and plan[0] is scorer and plan[2] == "own"
        assert batch._takes_history_batches(scorer, lookup) and batch._has_panels(scorer, lookup)
        parts = batch._bias_predict_parts(pipe)
        if fallback is None:  # (std:topn has no rating predictor)
            assert parts is None
        else:
            assert parts == (scorer, lookup, fallback)
        assert batch._batched_predict_parts(pipe) is None
        mode, ranker, route = batch._candidate_mode(pipe, {}, 3)
        assert mode == "topn" and route is plan or route == plan


def test_untrained_and_partial_models_keep_the_loop():
    from lkpy_amd import batch
    from lkpy_amd.basic import UserTrainingHistoryLookup

    data = _small()
    # untrained: nothing to route by
    pipe = _pipe(None, fallback=True)
    pipe.node("history-lookup").component.train(data)
    assert batch._candidate_route(pipe) is None and batch._bias_predict_parts(pipe) is None
    assert not batch._has_panels(pipe.node("scorer").component,
                                 pipe.node("history-lookup").component)
    # no item term: the model has no item vocabulary
    pipe = _pipe(data, fallback=False, entities=["user"])
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    assert scorer.model.items is None and scorer.model.users is not None
    assert batch._candidate_route(pipe) is None and batch._bias_predict_parts(pipe) is None
    assert not batch._takes_history_batches(scorer, lookup)
    # no user term: any lookup over the same items will do, ratings or not
    bare = _small(ratings=False)
    pipe = _pipe(data, fallback=False, lookup_data=bare, entities=["item"])
    assert batch._candidate_route(pipe)[2] == "own"
    assert batch._bias_predict_parts(pipe) is not None
    # a user term over a lookup without ratings, or with float64 ones: the loop
    for other in (bare, _small(dtype=np.float64)):
        pipe = _pipe(data, fallback=True, lookup_data=other)
        scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
        assert isinstance(lookup, UserTrainingHistoryLookup)
        assert batch._candidate_route(pipe) is None and batch._bias_predict_parts(pipe) is None
        assert not batch._takes_history_batches(scorer, lookup)
    # a dataset without ratings cannot train the scorer at all, as before
    with pytest.raises(KeyError):
        _pipe(bare, fallback=True)


def test_float64_ratings_are_fitted_on_the_host():
    "``device`` is not looked at when the ratings are not float32 (no GPU is needed to see it)"
    from lkpy_amd.basic import BiasModel

    data = _small(dtype=np.float64)
    m = BiasModel.learn(data, 5.0, device="cuda:0")
    g, ib, ub = R.parent_learn(data, 5.0)
    assert m.device_biases is None and m.global_bias == g
    assert R.same_bits(m.item_biases, ib) and R.same_bits(m.user_biases, ub)


def test_unknown_items_send_a_ranking_to_the_loop():
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer, PopScorer

    nums = np.array([3, -1, 4], np.int32)
    assert batch._ranks_unknown_items(BiasScorer(), nums=nums)
    assert not batch._ranks_unknown_items(BiasScorer(), nums=nums[[0, 2]])
    assert not batch._ranks_unknown_items(PopScorer(), nums=nums)


def test_golden_pipeline_file():
    from lkpy_amd.basic import BiasScorer, FallbackScorer
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(Path(__file__).resolve().parent / "golden" / "pipelines" /
                                "bias.toml")
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, BiasScorer) and scorer.config.damping == 50.0
    assert isinstance(pipe.node("rating-predictor").component, FallbackScorer)
    assert isinstance(pipe.node("fallback-predictor").component, BiasScorer)
