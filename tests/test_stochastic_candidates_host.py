"""CPU: what the stochastic / random candidate routes decide on the host -- the new keyword of
``recommend_samples``, how candidate lists are addressed and packed, and the address validation
of the device wrapper, which raises before any device call."""
import inspect

import numpy as np
import pytest


def test_recommend_samples_takes_candidates():
    from lkpy_amd import batch
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    sig = inspect.signature(batch.recommend_samples).parameters
    assert sig["candidates"].default is None and sig["candidates"].kind is sig["batch_size"].kind
    pipe = topn_pipeline(ImplicitMFScorer(features=4))
    pipe.replace_component("ranker", StochasticTopNRanker(rng=(7, "user")),
                           query="history-lookup")
    out = batch.recommend_samples(pipe, None, 5, 3, candidates={})
    assert len(out) == 0 and out.key_fields == ("user_id", "sample")
    with pytest.raises(ValueError, match=r"no candidates for user 4\b"):
        batch.recommend_samples(pipe, [4], 5, 3, candidates={})


def _offsets(lens):
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr


def test_candidate_addresses():
    from lkpy_amd.batch import _candidate_addresses
    from lkpy_amd.data import ItemList, Vocabulary

    vocab = Vocabulary(np.arange(100, 150), "item")
    other = Vocabulary(np.arange(100, 160), "item")
    ids = [np.array([140, 101, 120, 999]), np.zeros(0, np.int64), np.array([105]),
           np.array([149, 100])]
    flat = np.concatenate(ids)
    numbers = vocab.numbers(flat, missing="negative")
    offsets = _offsets([len(i) for i in ids])

    # id lists (and a frame, ``lists=None``): positions, as wide as the list
    for lists in ([ItemList(item_ids=i) for i in ids], None):
        addr, widths, order = _candidate_addresses(lists, offsets, numbers, vocab)
        assert order is None and addr.dtype == widths.dtype == np.int32
        assert addr.tolist() == [0, 1, 2, 3, 0, 0, 1] and widths.tolist() == [4, 0, 1, 2]

    # lists that carry the vocabulary: sorted numbers, as wide as the vocabulary, a permutation
    known = [i[i < 150] for i in ids]
    kflat = np.concatenate(known)
    knum = vocab.numbers(kflat)
    koff = _offsets([len(i) for i in known])
    lists = [ItemList(item_ids=i, vocabulary=vocab) for i in known]
    addr, widths, order = _candidate_addresses(lists, koff, knum, vocab)
    assert addr.tolist() == [1, 20, 40, 5, 0, 49] and widths.tolist() == [50] * 4
    assert order.dtype == np.int64 and order.tolist() == [1, 2, 0, 3, 5, 4]
    assert np.array_equal(knum[order], addr)  # sorted = original[order] ...
    back = np.empty_like(order)
    back[order] = np.arange(len(order))
    assert np.array_equal(addr[back], knum)  # ... and back again
    assert np.array_equal(np.searchsorted(koff, order, side="right"),
                          np.searchsorted(koff, np.arange(len(order)), side="right"))
    same = Vocabulary(np.arange(100, 150), "item")  # an equal vocabulary is the same one
    assert _candidate_addresses([ItemList(item_ids=i, vocabulary=same) for i in known], koff,
                                knum, vocab) is not None

    # for the loop: a repeated item (either kind), a foreign vocabulary, mixed lists
    twice = np.array([140, 101, 140])
    for lists in ([ItemList(item_ids=twice)], [ItemList(item_ids=twice, vocabulary=vocab)]):
        assert _candidate_addresses(lists, _offsets([3]), vocab.numbers(twice), vocab) is None
    # (an unknown item twice is no repeat: it takes no part; the same item in two lists is none)
    assert _candidate_addresses(None, _offsets([2]), np.array([-1, -1]), vocab) is not None
    assert _candidate_addresses(None, _offsets([1, 1]), np.array([7, 7]), vocab) is not None
    foreign = [ItemList(item_ids=i, vocabulary=other) for i in known]
    assert _candidate_addresses(foreign, koff, knum, vocab) is None
    mixed = [ItemList(item_ids=known[0], vocabulary=vocab), ItemList(item_ids=known[1]),
             ItemList(item_ids=known[2]), ItemList(item_ids=known[3], vocabulary=vocab)]
    assert _candidate_addresses(mixed, koff, knum, vocab) is None
    # an empty list is of either kind
    mixed[2] = ItemList(item_ids=known[2], vocabulary=vocab)
    assert _candidate_addresses(mixed, koff, knum, vocab) is not None


def test_addresses_are_validated_before_any_device_call(monkeypatch):
    from lkpy_amd import _device as D
    from lkpy_amd import _native
    from lkpy_amd.stochastic import rank_ragged

    def never(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", never)
    ptr, addr, widths = D.check_ragged_addresses([0, 3, 3, 5], [0, 2, 7, 1, 4], [8, 2, 5])
    assert ptr.dtype == np.int64 and addr.dtype == widths.dtype == np.int32
    D.check_ragged_addresses([0], [], [])
    D.check_ragged_addresses([0, 2, 4], [3, 4, 0, 1], [5, 5])  # a new segment may start lower
    scores = np.ones(5, np.float32)
    opts = dict(transform="softmax", scale=1.0, seed=1)
    bad = {
        "descending": ([0, 3, 3, 5], [0, 7, 2, 1, 4], [8, 2, 5], "ascend"),
        "repeated": ([0, 3, 3, 5], [0, 2, 2, 1, 4], [8, 2, 5], "ascend"),
        "too large": ([0, 3, 3, 5], [0, 2, 8, 1, 4], [8, 2, 5], "width"),
        "the next segment's width": ([0, 3, 3, 5], [0, 2, 7, 1, 5], [8, 2, 5], "width"),
        "negative": ([0, 3, 3, 5], [-1, 2, 7, 1, 4], [8, 2, 5], "width"),
        "offsets": ([0, 3, 2, 5], [0, 2, 7, 1, 4], [8, 2, 5], "tgt_ptr"),
        "one width short": ([0, 3, 3, 5], [0, 2, 7, 1, 4], [8, 5], "tgt_ptr"),
    }
    for name, (p, a, w, match) in bad.items():
        with pytest.raises(ValueError, match=match):
            D.ragged_stochastic_keys(p, a, scores, w, np.zeros(len(w), np.uint64), **opts)
        with pytest.raises(ValueError, match=match):
            rank_ragged(p, a, None, scores, w, np.zeros(len(w), np.uint64), 3, **opts)
