"""The stochastic ranker off the device: the Philox restatement's known answers, the order of the
log-domain key against the reference's key, the configuration, the seeding rules, and the path
``batch.recommend`` takes for a scorer without score panels."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import stochastic_restatement as R  # noqa: E402


def test_philox_known_answers():
    "Random123's known-answer vectors for Philox4x32-10"
    zero = R.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [f"{w:08x}" for w in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = R.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [f"{w:08x}" for w in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_uniform_is_exact_in_float32_and_open():
    bits = np.array([0, 1 << 9, 0xFFFFFFFF, 0x80000000, 12345678], np.uint32)
    u = R.uniform(bits)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    draws = R.random_bits(99, 5, 0, 10)
    assert np.array_equal(draws[:7], R.random_bits(99, 5, 0, 7))  # (not a function of the length)
    assert not np.array_equal(draws, R.random_bits(99, 5, 1, 10))
    assert not np.array_equal(draws, R.random_bits(99, 1 << 32 | 5, 0, 10))


@pytest.mark.parametrize("transform,scale", [("softmax", 1.0), ("softmax", 30.0), ("linear", 1.0),
                                             (None, 1.0)])
def test_order_of_g_is_order_of_reference_key(transform, scale):
    "descending g == descending log(u) / max(w, tiny), and the reference key is -exp(-g)"
    scores = np.random.default_rng(3).standard_normal(500).astype(np.float32)
    u = R.uniform(R.random_bits(1, 2, 0, 500))
    ref = R.reference_keys(scores, transform, scale, u)
    g = R.g64(scores, transform, scale, u)
    assert np.array_equal(R.stable_descending(g), R.stable_descending(ref))
    assert np.allclose(-np.exp(-g), ref, rtol=1e-12, atol=0)
    assert np.abs(R.g32(scores, transform, scale, u) - g).max() < 1e-4


def test_config_defaults_and_validation():
    from pydantic import ValidationError

    from lkpy_amd.stochastic import StochasticTopNConfig, StochasticTopNRanker

    cfg = StochasticTopNConfig()
    assert (cfg.n, cfg.rng, cfg.transform, cfg.scale) == (None, None, "softmax", 1.0)
    r = StochasticTopNRanker(n=5, transform=None, scale=2.5, rng=7)
    assert r.config.n == 5 and r.config.transform is None and r.config.scale == 2.5
    assert StochasticTopNRanker({"transform": "linear"}).config.transform == "linear"
    with pytest.raises(ValidationError):
        StochasticTopNRanker(transform="sigmoid")
    with pytest.raises(ValueError):
        StochasticTopNRanker(rng=(1, "item"))
    with pytest.raises(ValueError):
        StochasticTopNRanker(rng="item")
    assert r._length(None) == 5 and r._length(-1) == 5 and r._length(3) == 3
    assert StochasticTopNRanker()._length(None) == -1


def test_missing_scores_raise():
    from lkpy_amd.data import ItemList
    from lkpy_amd.stochastic import StochasticTopNRanker

    with pytest.raises(ValueError, match="scores"):
        StochasticTopNRanker(rng=1)(ItemList([1, 2, 3]))


def test_all_non_finite_scores_give_an_empty_ordered_list():
    from lkpy_amd.data import ItemList
    from lkpy_amd.stochastic import StochasticTopNRanker

    out = StochasticTopNRanker(rng=1)(ItemList([1, 2, 3], scores=[np.nan, np.inf, -np.inf]))
    assert len(out) == 0 and out.ordered


def test_seeding_rules():
    from lkpy_amd.stochastic import StochasticTopNRanker, user_stream

    want = int(np.random.SeedSequence(42).generate_state(1, np.uint64)[0])
    fixed = StochasticTopNRanker(rng=42)
    assert fixed.seed == want and not fixed.by_user
    # a fixed seed: (calls so far << 32) | row position -- a second call draws afresh
    assert fixed.streams(np.array([10, 20, 30])).tolist() == [0, 1, 2]
    assert fixed.streams(["a", "b"]).tolist() == [1 << 32, (1 << 32) | 1]
    assert fixed.streams(None, 1).tolist() == [2 << 32]
    # by user: the id itself, or the md5 fold of a str / bytes id; the call count does not matter
    by_user = StochasticTopNRanker(rng=(42, "user"))
    assert by_user.seed == want and by_user.by_user
    assert by_user.streams(np.array([10, -1])).tolist() == [10, 2 ** 64 - 1]
    assert by_user.streams(np.array([10, -1])).tolist() == [10, 2 ** 64 - 1]
    assert by_user.streams([np.int32(7), 8]).tolist() == [7, 8]
    from hashlib import md5

    fold = abs(int(np.bitwise_xor.reduce(np.frombuffer(md5(b"alice").digest(), np.int32))))
    assert user_stream("alice") == user_stream(b"alice") == fold
    assert by_user.streams(np.array(["alice", "bob"])).tolist() == [fold, user_stream("bob")]
    # a query without a user id takes a counted stream
    assert by_user.streams(None, 1).tolist() == [4 << 32]
    # a bare "user" and None draw fresh entropy
    assert StochasticTopNRanker(rng="user").by_user
    assert StochasticTopNRanker().seed != StochasticTopNRanker().seed
    assert StochasticTopNRanker(rng=np.random.SeedSequence(42)).seed == want


def test_batch_recommend_without_panels_takes_the_per_user_loop(monkeypatch):
    """A stochastic ranker over a scorer that has ``recommend_batch`` but no ``dense_scores_batch``:
    ``batch.recommend`` must not hand back the scorer's deterministic lists -- every user goes
    through ``pipe.run``, ranker included."""
    from lkpy_amd import batch
    from lkpy_amd.data import Dataset, ItemList
    from lkpy_amd.pipeline import Component, topn_pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    class Stub(Component):
        accepts_history_batch = True

        def __call__(self, query, items: ItemList) -> ItemList:
            return ItemList(items, scores=np.arange(len(items), dtype=np.float32))

        def recommend_batch(self, queries, n, **kw):
            raise AssertionError("the deterministic batch path was taken")

    ds = Dataset.from_arrays(np.array([1, 1, 2, 3]), np.array([10, 11, 12, 13]))
    pipe = topn_pipeline(Stub())
    pipe.train(ds)
    seen = []

    def ranked(self, items, query=None, n=None, *, include_weights=False):
        seen.append((query.user_id, n, len(items)))
        return items[:n]  # (no device here: the sampling itself is test_gpu_stochastic's)

    monkeypatch.setattr(StochasticTopNRanker, "__call__", ranked)
    pipe.replace_component("ranker", StochasticTopNRanker(rng=(3, "user")),
                           query="history-lookup")
    out = batch.recommend(pipe, [1, 2, 3], 2)
    assert seen == [(1, 2, 2), (2, 2, 3), (3, 2, 3)]  # (candidates: the items minus the history)
    assert out.key_fields == ("user_id",) and len(out) == 3 and len(out.lookup(2)) == 2
    with pytest.raises(TypeError):
        batch.recommend_samples(topn_pipeline(Stub()), [1], 2, 3)


def test_library_exports_the_stochastic_entry_points():
    from lkpy_amd import _native

    lib = _native.load()
    for name in ("lk_stochastic_row_stats", "lk_stochastic_keys", "lk_stochastic_key_of_bits"):
        assert name in _native.declared_symbols() and hasattr(lib, name)
