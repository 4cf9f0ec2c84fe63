"""CPU: the host side of per-query candidate lists -- the NumPy restatement of ``lk_ragged_topn`` /
``lk_panel_take_ragged`` against a brute-force loop and its ordering rules, the offset validation
of the device wrappers, and what ``batch.recommend(candidates=...)`` / ``batch.score`` decide and
raise before any device work.  User-kNN training is SciPy on the host, so no GPU is needed."""
import inspect
import math
import struct
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import candidates_restatement as R

GOLDEN = Path(__file__).parent / "golden"


def _key(x: float) -> int:
    "f2key of one float32, written out with struct: the brute-force side shares no code with R"
    (u,) = struct.unpack("<I", struct.pack("<f", x))
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _brute_topn(ptr, items, scores, n):
    rows = []
    for q in range(len(ptr) - 1):
        ent = [(t - ptr[q], items[t], scores[t]) for t in range(ptr[q], ptr[q + 1])
               if not math.isnan(scores[t]) and items[t] >= 0]
        done = []
        while ent and (n < 0 or len(done) < n):  # selection: the best of what is left
            best = ent[0]
            for e in ent[1:]:
                if _key(e[2]) > _key(best[2]):  # (equal keys: the earlier position stays)
                    best = e
            ent.remove(best)
            done.append(best)
        rows.append(done)
    return rows


def _ptr(lens):
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr


def test_restatement_against_a_brute_force_loop(rng):
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0, -3.5], np.float32)
    for trial in range(20):
        lens = rng.integers(0, 9, 6)
        ptr = _ptr(lens)
        scores = rng.standard_normal(int(ptr[-1])).astype(np.float32)
        pick = rng.random(len(scores)) < 0.5
        scores[pick] = rng.choice(special, int(pick.sum()))
        items = rng.integers(-1, 5, len(scores)).astype(np.int32)
        for n in (-1, 0, 1, 3, 12):
            idx, sc = R.ragged_topn_ref(ptr, items, scores, n)
            width = int(lens.max()) if n < 0 else n
            assert idx.shape == sc.shape == (6, width)
            for q, row in enumerate(_brute_topn(ptr.tolist(), items.tolist(), scores.tolist(), n)):
                m = len(row)
                assert idx[q, :m].tolist() == [e[1] for e in row]
                assert R.bits(sc[q, :m]).tolist() == \
                    R.bits(np.array([e[2] for e in row], np.float32)).tolist()
                assert (idx[q, m:] == -1).all() and np.isnan(sc[q, m:]).all()
    panel = rng.standard_normal((3, 7)).astype(np.float32)
    ptr, items = _ptr([2, 0, 3]), np.array([6, 7, -1, 0, 4], np.int32)
    want = [panel[0, 6], np.nan, np.nan, panel[2, 0], panel[2, 4]]
    assert np.array_equal(R.take_ragged_ref(panel, 7, ptr, items), np.array(want, np.float32),
                          equal_nan=True)
    assert np.isnan(R.take_ragged_ref(panel, 6, ptr, items)[0])  # 6 is outside [0, 6)


def test_ordering_rules():
    ptr = _ptr([5, 4, 3, 4, 3])
    items = np.array([10, 11, 12, 13, 14, 1, 2, 3, 4, 5, 6, 7, 9, 9, 3, -1, 8, 20, 21], np.int32)
    scores = np.array([-0.0, 0.0, 1.0, 0.0, -0.0,            # the zeros tie: positions decide
                       -np.inf, 5.0, np.inf, -np.inf,        # +-inf are valid scores
                       np.nan, np.nan, np.nan,               # nothing left
                       1.0, 2.0, 1.0, 9.0,                   # a repeated item; a negative item
                       0.5, np.nan, 0.5], np.float32)        # NaN dropped, the tie keeps order
    idx, sc = R.ragged_topn_ref(ptr, items, scores, -1)
    assert idx.shape == (5, 5)
    assert idx[0].tolist() == [12, 10, 11, 13, 14]
    assert R.bits(sc[0]).tolist() == [0x3F800000, 0x80000000, 0, 0, 0x80000000]
    assert idx[1].tolist() == [3, 2, 1, 4, -1] and sc[1, 0] == np.inf and sc[1, 3] == -np.inf
    assert (idx[2] == -1).all() and np.isnan(sc[2]).all()
    assert idx[3].tolist() == [9, 9, 3, -1, -1] and sc[3, :3].tolist() == [2.0, 1.0, 1.0]
    assert idx[4].tolist() == [8, 21, -1, -1, -1]
    top2, _ = R.ragged_topn_ref(ptr, items, scores, 2)
    assert np.array_equal(top2, idx[:, :2])
    assert R.f2key([-0.0])[0] == R.f2key([0.0])[0] == 0x80000000
    keys = R.f2key([-np.inf, -1.0, -0.0, 1e-30, 1.0, np.inf]).astype(np.int64)
    assert (np.diff(keys) > 0).all() and keys[0] > 0


def test_offsets_are_validated_on_the_host():
    from lkpy_amd import _device as D

    assert D.check_ragged([0, 2, 2, 5], 3, 5).dtype == np.int64
    for bad, nq, total in (([0, 3, 2, 5], 3, 5), ([1, 2, 3, 5], 3, 5), ([0, 2, 4], 3, 4),
                           ([0, 2, 2, 4], 3, 5)):
        with pytest.raises(ValueError, match="tgt_ptr"):
            D.check_ragged(bad, nq, total)


# ---- the public interface ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def uknn_pipe(ml_ds):
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import topn_pipeline

    pipe = topn_pipeline(UserKNNScorer(k=20))
    pipe.train(ml_ds)
    return pipe


class _BatchReranker:
    "a reranker that takes whole batches; never reached by the tests below"
    vocab = None

    def __call__(self, items, n=None):
        raise AssertionError("the reranker was run")

    def rerank_batch(self, idx, sc, n):
        raise AssertionError("the reranker was run")


def _no_device(monkeypatch, pipe):
    from lkpy_amd import _native

    def never(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", never)
    monkeypatch.setattr(pipe.node("history-lookup").component, "batch", never, raising=False)
    monkeypatch.setattr(pipe, "run", never, raising=False)


def test_score_is_a_public_entry_point():
    from lkpy_amd import batch

    sig = inspect.signature(batch.score)
    assert list(sig.parameters)[:2] == ["pipe", "test"] and "batch_size" in sig.parameters
    rec = inspect.signature(batch.recommend).parameters
    assert rec["candidates"].default is None and rec["candidates"].kind is rec["batch_size"].kind


def test_a_user_without_candidates_is_an_error(ml_ds, uknn_pipe, monkeypatch):
    from lkpy_amd import batch

    uids = [int(u) for u in ml_ds.users.ids()[:3]]
    cand = {uids[0]: ml_ds.items.ids()[:5], uids[1]: ml_ds.items.ids()[5:9]}
    _no_device(monkeypatch, uknn_pipe)
    with pytest.raises(ValueError, match=rf"no candidates for user {uids[2]}\b"):
        batch.recommend(uknn_pipe, [uids[1], uids[2], 987654321], 10, candidates=cand)


def test_rerank_depth_below_n_is_an_error(ml_ds, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import topn_pipeline

    pipe = topn_pipeline(UserKNNScorer(k=20), reranker=_BatchReranker())
    pipe.train(ml_ds)
    uid = int(ml_ds.users.ids()[0])
    cand = {uid: ml_ds.items.ids()[:50]}
    _no_device(monkeypatch, pipe)
    with pytest.raises(ValueError, match="rerank_depth = 5 is below n = 10"):
        batch.recommend(pipe, None, 10, candidates=cand, rerank_depth=5)
    plain = topn_pipeline(UserKNNScorer(k=20))
    with pytest.raises(ValueError, match="rerank_depth needs"):
        batch.recommend(plain, None, 10, candidates=cand, rerank_depth=20)


def test_routes(ml_ds, uknn_pipe):
    from lkpy_amd import batch
    from lkpy_amd.als import BiasedMFScorer, ImplicitMFScorer
    from lkpy_amd.data import Dataset
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import Pipeline, topn_pipeline

    scorer, lookup, route = batch._candidate_route(uknn_pipe)
    assert route == "panel" and scorer is uknn_pipe.node("scorer").component
    assert lookup is uknn_pipe.node("history-lookup").component
    # an untrained scorer, an empty scorer slot, explicit feedback without ratings: the loop
    assert batch._candidate_route(topn_pipeline(ImplicitMFScorer(features=4))) is None
    assert batch._candidate_route(Pipeline.std_topn()) is None
    bare = Dataset(ml_ds.users, ml_ds.items, ml_ds._rows, ml_ds._cols, {})
    explicit = topn_pipeline(uknn_pipe.node("scorer").component)
    explicit.node("history-lookup").component.train(bare)
    assert batch._candidate_route(explicit) is None
    implicit = topn_pipeline(UserKNNScorer(k=20, feedback="implicit"))
    implicit.train(bare)
    assert batch._candidate_route(implicit)[2] == "panel"
    # a lookup over another item vocabulary than the scorer's
    other = Dataset.from_arrays(ml_ds.users.ids()[ml_ds._rows[:4000]],
                                ml_ds.items.ids()[ml_ds._cols[:4000]] + 5_000_000,
                                np.asarray(ml_ds._attrs["rating"][:4000]))
    mixed = topn_pipeline(uknn_pipe.node("scorer").component)
    mixed.node("history-lookup").component.train(other)
    assert batch._candidate_route(mixed) is None
    # the scorers with a method of their own take it; BiasedMFScorer has none and no panel route
    assert hasattr(ImplicitMFScorer, "score_candidates_batch")
    assert not hasattr(BiasedMFScorer, "score_candidates_batch")


def test_loop_follows_users_and_candidates(ml_ds, monkeypatch):
    "the per-query fallback: lists re-ordered by ``users``, a frame split per user, ``n`` passed on"
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList, ItemListCollection
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.std_topn()  # an empty scorer slot: no route
    calls = []

    def run(node, **kw):
        calls.append((node, kw["query"], kw.get("n")))
        return kw["items"]

    monkeypatch.setattr(pipe, "run", run, raising=False)
    cand = {7: ItemList(np.array([1, 2, 3])), 8: ItemList(np.array([], np.int64)),
            9: ItemList(np.array([4]))}
    out = batch.recommend(pipe, [9, 7], None, candidates=cand)
    assert [k.user_id for k in out.keys()] == [9, 7]
    assert out.lookup(9).ids().tolist() == [4] and out.lookup(7).ids().tolist() == [1, 2, 3]
    assert calls == [("recommender", 9, None), ("recommender", 7, None)]
    out = batch.recommend(pipe, None, 2, candidates=cand)
    assert [k.user_id for k in out.keys()] == [7, 8, 9] and len(out.lookup(8)) == 0
    frame = pd.DataFrame({"user_id": [5, 6, 5, 6, 6], "item_id": [1, 2, 3, 4, 5]})
    out = batch.recommend(pipe, [6, 5], 2, candidates=frame)
    assert out.lookup(6).ids().tolist() == [2, 4, 5] and out.lookup(5).ids().tolist() == [1, 3]
    ilc = ItemListCollection.from_dict(cand, key=("user_id",))
    out = batch.recommend(pipe, [8, 9], 2, candidates=ilc)
    assert [k.user_id for k in out.keys()] == [8, 9] and out.lookup(9).ids().tolist() == [4]
    calls.clear()
    out = batch.score(pipe, cand)
    assert [c[0] for c in calls] == ["scorer"] * 3 and out.lookup(7).ids().tolist() == [1, 2, 3]
