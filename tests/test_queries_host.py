"""CPU: the scorers' one host-side query packer (``lkpy_amd._queries``), option by option."""
import numpy as np
import pytest

from lkpy_amd._queries import (item_scores, pack_histories, pack_targets, resolve_queries,
                               user_numbers)
from lkpy_amd.basic import HistoryBatch
from lkpy_amd.data import ItemList, RecQuery, Vocabulary

ITEMS = Vocabulary(np.array([10, 20, 30, 40]))
MEANS = np.array([0.5, 1.5, 2.5, 3.5], dtype=np.float32)


def _queries(ratings: bool = True):
    "unsorted with an unknown item | user id only | empty list | unknown only | a repeat"
    r = (lambda *v: {"rating": np.array(v, dtype=np.float64)}) if ratings else (lambda *v: {})
    return [RecQuery(user_items=ItemList([30, 999, 10], **r(4.0, 2.0, 5.0))),
            RecQuery(user_id=5),
            RecQuery(user_items=ItemList(np.zeros(0, np.int64))),
            RecQuery(user_items=ItemList([999], **r(3.0))),
            RecQuery(user_items=ItemList([20, 20, 40], **r(1.0, 2.0, 3.5)))]


def _als(**cfg):
    from lkpy_amd.als import ImplicitMFConfig, ImplicitMFScorer

    sc = ImplicitMFScorer(ImplicitMFConfig(**cfg))
    sc.items = ITEMS
    return sc


def _iknn(feedback):
    from lkpy_amd.knn import ItemKNNScorer

    sc = ItemKNNScorer(feedback=feedback)
    sc.items, sc.item_means = ITEMS, MEANS
    return sc


KEEP_PTR, KEEP_IDX = [0, 3, 3, 3, 4, 7], [2, -1, 0, -1, 1, 1, 3]
DROP_PTR, DROP_IDX = [0, 2, 2, 2, 2, 5], [0, 2, 1, 1, 3]
TABLE = {
    # ALS: rating * weight (2.0), rows sorted by item number with the values following
    "als": (lambda qs: _als(weight=2.0, use_ratings=True)._history_rows(qs),
            DROP_PTR, DROP_IDX, [10.0, 8.0, 2.0, 4.0, 7.0]),
    "flexmf": (lambda qs: pack_histories(qs, ITEMS, unknown="drop", sort=True),
               DROP_PTR, DROP_IDX, None),
    # item-kNN explicit: rating - mean in query order, the unknown items' 2.0 and 3.0 as they are
    "iknn-explicit": (lambda qs: pack_histories(qs, ITEMS, unknown="keep",
                                                values=_iknn("explicit")._centred_ratings),
                      KEEP_PTR, KEEP_IDX, [1.5, 2.0, 4.5, 3.0, -0.5, 0.5, 0.0]),
    "iknn-implicit": (lambda qs: pack_histories(qs, ITEMS, unknown="keep"),
                      KEEP_PTR, KEEP_IDX, None),
    "slim": (lambda qs: pack_histories(qs, ITEMS, unknown="keep"), KEEP_PTR, KEEP_IDX, None),
    "ease": (lambda qs: pack_histories(qs, ITEMS, unknown="drop", unique=True),
             [0, 2, 2, 2, 2, 4], [0, 2, 1, 3], None),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_pack_histories_table(name):
    pack, want_ptr, want_idx, want_val = TABLE[name]
    ptr, idx, val = pack(_queries())
    assert ptr.dtype == np.int64 and ptr.tolist() == want_ptr
    assert idx.dtype == np.int32 and idx.tolist() == want_idx
    if want_val is None:
        assert val is None
    else:
        assert val.dtype == np.float32 and val.tolist() == want_val


def test_pack_histories_without_queries_or_entries():
    for qs in ([], _queries()[1:3]):
        ptr, idx, val = pack_histories(qs, ITEMS, unknown="keep", values=lambda h, n, k: 1 / 0)
        assert ptr.dtype == np.int64 and ptr.tolist() == [0] * (len(qs) + 1)
        assert idx.dtype == np.int32 and len(idx) == 0
        assert val.dtype == np.float32 and len(val) == 0  # (values asked for: an empty array)
    with pytest.raises(ValueError):
        pack_histories([], ITEMS, unknown="ignore")


def test_als_confidence_arithmetic():
    "constant weight; rating * weight reordered; the product formed in float64, cast once"
    ptr, idx, val = _als(weight=40.0)._history_rows(_queries(ratings=False))
    assert ptr.tolist() == DROP_PTR and idx.tolist() == DROP_IDX
    assert val.dtype == np.float32 and val.tolist() == [40.0] * 5
    q = [RecQuery(user_items=ItemList([20, 10], rating=np.array([3.0, 5.0])))]
    _, idx, val = _als(weight=2.0, use_ratings=True)._history_rows(q)
    assert idx.tolist() == [0, 1] and val.tolist() == [10.0, 6.0]
    r, w = 3.3, 2.1
    assert np.float32(np.float64(r) * w) != np.float32(r) * np.float32(w)  # (the pair tells)
    q = [RecQuery(user_items=ItemList([20], rating=np.array([r], dtype=np.float64)))]
    _, _, val = _als(weight=w, use_ratings=True)._history_rows(q)
    assert val.dtype == np.float32 and val[0] == np.float32(np.float64(r) * w)


def test_missing_ratings_errors_keep_type_and_text():
    qs = _queries(ratings=False)
    with pytest.raises(ValueError, match=r"^no ratings in user items$"):
        _als(use_ratings=True)._history_rows(qs)
    with pytest.raises(RuntimeError, match=r"^explicit-feedback scorer must have ratings$"):
        pack_histories(qs, ITEMS, unknown="keep", values=_iknn("explicit")._centred_ratings)
    # no history to take ratings from: nothing to complain about
    assert _als(use_ratings=True)._history_rows(qs[1:3])[0].tolist() == [0, 0, 0]


class _Batch(HistoryBatch):
    "a HistoryBatch without a lookup behind it: the attributes the helpers read"

    def __init__(self, items=ITEMS, users=None, user_ids=(), user_nums=()):
        self.items, self.users = items, users
        self.user_ids = np.asarray(user_ids)
        self.user_nums = np.asarray(user_nums, dtype=np.int32)

    def queries(self):
        return ["per-query"]


def test_user_numbers():
    users = Vocabulary(np.array([7, 8, 9]))
    qs = [RecQuery(user_id=8), RecQuery(user_id=77), RecQuery(user_items=ItemList([10]))]
    got = user_numbers(qs, users)
    assert got.dtype == np.int64 and got.tolist() == [1, -1, -1]
    # the batch's own numbers are taken when its vocabulary is the scorer's (they are not looked
    # up again: these deliberately disagree with the ids) ...
    for vocab in (users, Vocabulary(np.array([7, 8, 9]))):
        got = user_numbers(_Batch(users=vocab, user_ids=[9, 7, 1], user_nums=[0, 1, -1]), users)
        assert got.dtype == np.int64 and got.tolist() == [0, 1, -1]
    # ... and looked up by id when it is another one
    other = _Batch(users=Vocabulary(np.array([1, 7, 9])), user_ids=[9, 7, 1], user_nums=[2, 1, 0])
    got = user_numbers(other, users)
    assert got.dtype == np.int64 and got.tolist() == [2, 0, -1]
    for q in (qs, other):
        got = user_numbers(q, None)
        assert got.dtype == np.int64 and got.tolist() == [-1, -1, -1]


def test_item_scores():
    row = np.array([0.25, 0.5, 0.75, 1.0])  # float64 in, float32 out
    got = item_scores(ItemList([40, 999, 10, 40]), ITEMS, row)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([1.0, np.nan, 0.25, 1.0], np.float32), equal_nan=True)
    got = item_scores(ItemList(np.zeros(0, np.int64)), ITEMS, row)
    assert got.dtype == np.float32 and got.shape == (0,)


def test_pack_targets():
    ptr, nums = pack_targets([], ITEMS)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0]
    assert nums.dtype == np.int32 and nums.shape == (0,)
    empty = ItemList(np.zeros(0, np.int64))
    ptr, nums = pack_targets([empty, empty], ITEMS)
    assert ptr.tolist() == [0, 0, 0] and nums.dtype == np.int32 and nums.shape == (0,)
    # an empty list between two others; an unknown id in its place; a repeat kept; list order kept
    lists = [ItemList([40, 999, 10]), empty, ItemList([20, 20, 30]),
             ItemList(item_nums=[3, 0], vocabulary=ITEMS)]
    ptr, nums = pack_targets(lists, ITEMS)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 3, 3, 6, 8]
    assert nums.dtype == np.int32 and nums.tolist() == [3, -1, 0, 1, 1, 2, 3, 0]
    assert nums.flags.c_contiguous and nums.flags.writeable  # (what torch.from_numpy takes)


def test_pack_targets_equals_the_per_list_lookup():
    rng = np.random.default_rng(5)
    vocab = Vocabulary(rng.permutation(np.arange(100, 130)))  # 30 items, numbered out of id order
    lists = [ItemList(rng.integers(95, 135, size=rng.integers(0, 12)))  # unknown ids, repeats
             for _ in range(50)]
    assert any(len(il) == 0 for il in lists)
    per_list = [il.numbers(vocabulary=vocab, missing="negative") for il in lists]
    assert any((p < 0).any() for p in per_list)
    assert any(len(np.unique(p)) < len(p) for p in per_list)
    ptr, nums = pack_targets(lists, vocab)
    assert ptr.dtype == np.int64 and nums.dtype == np.int32
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in per_list])]).tolist()
    assert np.array_equal(nums, np.concatenate(per_list))
    for i, p in enumerate(per_list):
        assert np.array_equal(nums[ptr[i]:ptr[i + 1]], p)


def test_resolve_queries():
    for vocab in (ITEMS, Vocabulary(np.array([10, 20, 30, 40]))):
        batch = _Batch(items=vocab)
        assert resolve_queries(batch, ITEMS) is batch
    assert resolve_queries(_Batch(items=Vocabulary(np.array([10, 20]))), ITEMS) == ["per-query"]
    q = RecQuery(user_id=3)
    got = resolve_queries([q, 5, ItemList([10])], ITEMS)
    assert got[0] is q and all(isinstance(g, RecQuery) for g in got)
    assert got[1].user_id == 5 and got[2].query_items.ids().tolist() == [10]
