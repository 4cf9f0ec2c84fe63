"""GPU, end to end on a 60-user x 400-item synthetic: ``batch.recommend(candidates=)`` and
``batch.recommend_samples(candidates=)`` for the stochastic ranker and the random pipeline against
the per-query pipeline -- ids, score bits and fields equal for every query, with ``pipe.run`` made
to raise wherever the batched route has to be the one taken."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TOP = 10
N_USERS, N_ITEMS = 60, 400
USER0, ITEM0 = 1000, 5000
RNG = (7, "user")
SCORERS = ("implicit-mf", "ease")
ROUTES = {"implicit-mf": "own", "ease": "panel"}


@pytest.fixture(scope="module")
def ds():
    from lkpy_amd.data import Dataset

    rng = np.random.default_rng(17)
    mask = rng.random((N_USERS, N_ITEMS)) < 0.08
    mask[np.arange(N_USERS), rng.integers(0, N_ITEMS, N_USERS)] = True
    rows, cols = np.nonzero(mask)
    return Dataset.from_arrays(rows + USER0, cols + ITEM0,
                               rng.integers(1, 11, len(rows)).astype(np.float32) / 2,
                               all_item_ids=np.arange(N_ITEMS) + ITEM0)


_PIPES: dict = {}


@pytest.fixture()
def pipe(request, gpu, ds):
    "one trained pipeline per scorer; every test puts the ranker it needs into it"
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    name = request.param
    if name not in _PIPES:
        scorer = {"implicit-mf": lambda: ImplicitMFScorer(features=8, epochs=2),
                  "ease": lambda: EASEScorer(regularization=2.0)}[name]()
        p = topn_pipeline(scorer, name=name)
        p.train(ds, TrainingOptions(rng=11))
        _PIPES[name] = p
    return _PIPES[name]


@pytest.fixture(scope="module")
def cand():
    """ids per user: 12 training users with 40 items and an unknown one, a list shorter than n, an
    empty one, one item, the whole catalogue, an unknown user"""
    rng = np.random.default_rng(23)
    items = np.arange(N_ITEMS) + ITEM0
    out = {}
    for u in range(USER0, USER0 + 24, 2):
        out[u] = np.concatenate([rng.choice(items, 40, replace=False), [77]])[rng.permutation(41)]
    out[USER0 + 31] = rng.choice(items, 3, replace=False)
    out[USER0 + 33] = np.zeros(0, items.dtype)
    out[USER0 + 35] = items[123:124]
    out[USER0 + 37] = items
    out[99999] = rng.choice(items, 40, replace=False)
    return out


def _id_lists(cand):
    from lkpy_amd.data import ItemList

    return {u: ItemList(item_ids=c) for u, c in cand.items()}


def _vocab_lists(cand, vocab):
    from lkpy_amd.data import ItemList

    return {u: ItemList(item_ids=c[c >= ITEM0], vocabulary=vocab) for u, c in cand.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stochastic(pipe, transform, rng=RNG):
    from lkpy_amd.stochastic import StochasticTopNRanker

    pipe.replace_component("ranker", StochasticTopNRanker(rng=rng, transform=transform, scale=2.0),
                           query="history-lookup")
    return pipe.node("ranker").component


def _forbid_run(monkeypatch, pipe):
    def never(*a, **k):
        raise AssertionError("the per-query loop was entered")

    monkeypatch.setattr(pipe, "run", never, raising=False)
    monkeypatch.setattr(pipe, "run_all", never, raising=False)


def _assert_same(got, want, users, *, scores=True):
    assert [k.user_id for k in got.keys()] == list(users)
    for u in users:
        g, w = got.lookup(u), want[u]
        assert np.array_equal(g.ids(), w.ids()), (u, g.ids(), w.ids())
        assert set(g._fields) == set(w._fields), (u, set(g._fields), set(w._fields))
        if scores:
            assert np.array_equal(_bits(g.scores()), _bits(w.scores())), u
        else:
            assert g.scores() is None and w.scores() is None


@pytest.mark.parametrize("transform", ["softmax", "linear"])
@pytest.mark.parametrize("kind", ["ids", "vocabulary"])
@pytest.mark.parametrize("pipe", SCORERS, indirect=True)
def test_recommend_candidates_samples_like_the_pipeline(pipe, cand, kind, transform, monkeypatch):
    from lkpy_amd import batch

    _stochastic(pipe, transform)
    assert batch._candidate_route(pipe)[2] == ROUTES[pipe.name]
    lists = _id_lists(cand) if kind == "ids" else \
        _vocab_lists(cand, pipe.node("scorer").component.items)
    users = list(lists)
    want = {u: pipe.run("recommender", query=u, items=lists[u], n=N_TOP) for u in users}
    everything = {u: pipe.run("recommender", query=u, items=lists[u], n=None) for u in users[:6]}
    with monkeypatch.context() as m:
        _forbid_run(m, pipe)
        got = batch.recommend(pipe, None, N_TOP, candidates=lists)
        some = [99999, USER0 + 37, USER0 + 4, USER0 + 33, USER0]
        picked = batch.recommend(pipe, some, N_TOP, candidates=lists, batch_size=2)
        ranked = batch.recommend(pipe, users[:6], None, candidates=lists)
    _assert_same(got, want, users)
    _assert_same(picked, want, some)
    _assert_same(ranked, everything, users[:6])
    assert len(got.lookup(99999)) == 0 and len(got.lookup(USER0 + 33)) == 0
    assert len(got.lookup(USER0 + 31)) == 3 and len(got.lookup(USER0 + 37)) == N_TOP
    assert len(got.lookup(USER0)) == N_TOP and 77 not in got.lookup(USER0).ids()
    assert len(ranked.lookup(USER0)) == 40
    assert (np.diff(got.lookup(USER0).scores()) <= 0).all()  # the keys, descending
    with pytest.raises(ValueError, match="no candidates for user 5"):
        batch.recommend(pipe, [USER0, 5], N_TOP, candidates=lists)
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(pipe, None, N_TOP, candidates=lists, rerank_depth=20)


@pytest.mark.parametrize("pipe", ["implicit-mf"], indirect=True)
def test_a_repeated_item_takes_the_loop(pipe, cand, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    _stochastic(pipe, "softmax")
    lists = _id_lists({u: cand[u] for u in (USER0, USER0 + 2, USER0 + 31)})
    twice = cand[USER0 + 2].copy()
    twice[5] = twice[11]
    lists[USER0 + 2] = ItemList(item_ids=twice)
    want = {u: pipe.run("recommender", query=u, items=lists[u], n=N_TOP) for u in lists}
    runs = []
    run = pipe.run
    monkeypatch.setattr(pipe, "run", lambda *a, **k: runs.append(k["query"]) or run(*a, **k),
                        raising=False)
    got = batch.recommend(pipe, None, N_TOP, candidates=lists)
    assert runs == list(lists)
    _assert_same(got, want, list(lists))


@pytest.mark.parametrize("pipe", SCORERS, indirect=True)
def test_recommend_samples_candidates(pipe, cand, monkeypatch):
    from lkpy_amd import batch

    ranker = _stochastic(pipe, "softmax")
    lists = _id_lists(cand)
    users = list(lists)
    S = 4
    want = {}
    for u in users:
        got = pipe.run_all("history-lookup", "scorer", query=u, items=lists[u])
        want[u] = ranker.sample(got["scorer"], got["history-lookup"], N_TOP, samples=S)
    with monkeypatch.context() as m:
        _forbid_run(m, pipe)
        out = batch.recommend_samples(pipe, None, N_TOP, S, candidates=lists)
        first = batch.recommend(pipe, None, N_TOP, candidates=lists)
        some = batch.recommend_samples(pipe, [USER0 + 37, 99999, USER0], N_TOP, 2,
                                       candidates=lists, batch_size=2)
    assert out.key_fields == ("user_id", "sample") and len(out) == S * len(users)
    assert [tuple(k) for k in out.keys()] == [(u, s) for u in users for s in range(S)]
    for u in users:
        for s in range(S):
            g, w = out.lookup(u, s), want[u][s]
            assert np.array_equal(g.ids(), w.ids()), (u, s)
            assert np.array_equal(_bits(g.scores()), _bits(w.scores())), (u, s)
        assert np.array_equal(out.lookup(u, 0).ids(), first.lookup(u).ids())
        assert np.array_equal(_bits(out.lookup(u, 0).scores()), _bits(first.lookup(u).scores()))
    assert not np.array_equal(out.lookup(USER0, 1).ids(), out.lookup(USER0, 2).ids())
    assert [tuple(k) for k in some.keys()] == [(u, s) for u in (USER0 + 37, 99999, USER0)
                                               for s in range(2)]
    assert np.array_equal(some.lookup(USER0, 1).ids(), want[USER0][1].ids())


@pytest.mark.parametrize("pipe", ["implicit-mf"], indirect=True)
def test_counted_streams_number_the_rows_of_one_call(pipe, cand, gpu, monkeypatch):
    "``rng=11``: stream = (calls so far << 32) | row, one call for the whole batch"
    import torch

    from lkpy_amd import batch
    from lkpy_amd.stochastic import StochasticTopNRanker, rank_panel

    ranker = _stochastic(pipe, "softmax", rng=11)
    twin = StochasticTopNRanker(rng=11, transform="softmax", scale=2.0)
    assert not ranker.by_user and twin.seed == ranker.seed
    ranker.streams(None, 3), twin.streams(None, 3)  # (both have made one call already)
    lists = _id_lists(cand)
    users = list(lists)
    scored = {u: pipe.run("scorer", query=u, items=lists[u]) for u in users}
    with monkeypatch.context() as m:
        _forbid_run(m, pipe)
        got = batch.recommend(pipe, None, N_TOP, candidates=lists, batch_size=5)
    assert ranker.calls == 2
    streams = twin.streams(np.asarray(users))
    assert streams.tolist() == [(1 << 32) | r for r in range(len(users))]
    width = max(len(c) for c in cand.values())
    panel = np.full((len(users), width), np.nan, np.float32)
    for r, u in enumerate(users):  # lists without a vocabulary: addressed by position
        panel[r, :len(cand[u])] = scored[u].scores()
    for r, u in enumerate(users):  # (a row is as wide as its own list)
        row = torch.from_numpy(panel[r:r + 1, :max(len(cand[u]), 1)].copy()).to(gpu)
        idx, keys = rank_panel(row, streams[r:r + 1], N_TOP, transform="softmax", scale=2.0,
                               seed=twin.seed)
        keep = idx[0, 0] >= 0
        g = got.lookup(u)
        assert np.array_equal(g.ids(), np.asarray(cand[u])[idx[0, 0][keep]]), u
        assert np.array_equal(_bits(g.scores()), _bits(keys[0, 0][keep])), u


@pytest.mark.parametrize("kind", ["ids", "vocabulary", "fields"])
def test_random_pipeline_over_candidates(gpu, ds, cand, kind, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import random_pipeline

    pipe = random_pipeline(rng=RNG)
    pipe.train(ds)
    if kind == "vocabulary":
        lists = _vocab_lists(cand, ds.items)
    elif kind == "fields":
        lists = {u: ItemList(item_ids=c, tag=np.arange(len(c)) * 3) for u, c in cand.items()}
    else:
        lists = _id_lists(cand)
    users = list(lists)
    want = {u: pipe.run("recommender", query=u, items=lists[u], n=N_TOP) for u in users}
    everything = {u: pipe.run("recommender", query=u, items=lists[u], n=None) for u in users}
    with monkeypatch.context() as m:
        _forbid_run(m, pipe)
        got = batch.recommend(pipe, None, N_TOP, candidates=lists)
        some = [99999, USER0 + 37, USER0 + 4, USER0 + 33, USER0]
        picked = batch.recommend(pipe, some, N_TOP, candidates=lists, batch_size=2)
        ranked = batch.recommend(pipe, None, None, candidates=lists)
    _assert_same(got, want, users, scores=False)
    _assert_same(picked, want, some, scores=False)
    _assert_same(ranked, everything, users, scores=False)
    if kind == "fields":
        for u in users:
            assert np.array_equal(got.lookup(u).field("tag"), want[u].field("tag"))
    # unknown users and unknown items are ordinary here
    assert len(got.lookup(99999)) == N_TOP and len(got.lookup(USER0 + 33)) == 0
    assert len(ranked.lookup(USER0)) == len(lists[USER0])
    if kind != "vocabulary":
        assert 77 in ranked.lookup(USER0).ids()
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(pipe, None, N_TOP, candidates=lists, rerank_depth=20)
