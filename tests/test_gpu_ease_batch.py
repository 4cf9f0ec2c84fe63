"""
EASE through the batch paths: the ``native`` solver of ``EASEScorer.train`` against the oracle,
``lk_ease_score_panel`` against ``lk_ease_score_batch`` bit for bit, and ``recommend_batch`` /
``batch.recommend`` / ``recommend_samples`` / ``rerank_depth`` on a ``topn_pipeline(EASEScorer)``
against one pipeline run per user.

Both paths see a history in ascending item order -- a ``HistoryBatch`` row is a training row, and
``pack_histories(..., unique=True)`` sorts (``np.unique``; asserted below) -- so the sums have the
same order and the scores are compared by their bits.
"""
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

N_TOP = 10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rand_binary(n_users, n_items, density, seed):
    m = sps.random(n_users, n_items, density=density, random_state=np.random.default_rng(seed),
                   format="csr", dtype=np.float32)
    m.data[:] = 1.0
    return sps.csr_array(m)


def _dataset(n_users, n_items, density, seed):
    from lkpy_amd.data import Dataset

    coo = _rand_binary(n_users, n_items, density, seed).tocoo()
    return Dataset.from_arrays(coo.row + 1000, coo.col + 10, np.ones(coo.nnz, np.float32))


# ---- training -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_items", [150, 300])
def test_native_solver_vs_oracle(gpu, oracle, n_items):
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.training import TrainingOptions

    ds = _dataset(400, n_items, 0.06, seed=n_items)
    algo = EASEScorer(regularization=1.0)
    algo.train(ds, TrainingOptions(environment={"LK_EASE_SOLVER": "native"}))
    mat = ds.interactions().matrix().scipy(attribute=None).astype(np.float32)
    want = oracle.ease_train(sps.csr_array(mat), 1.0)
    assert algo.weights.shape == want.shape and np.all(np.diag(algo.weights) == 0.0)
    rel = np.linalg.norm(algo.weights - want) / np.linalg.norm(want)
    print(f"native weights vs oracle at {n_items} items: rel = {rel:.3e}")
    assert rel < 1e-4, rel
    # the matrix training left in HBM is the device copy: nothing is uploaded for scoring
    dev = algo._device_weights()
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(algo.weights))


def test_default_solver_is_still_torch(gpu, monkeypatch):
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.training import TrainingOptions

    monkeypatch.delenv("LK_EASE_SOLVER", raising=False)
    ds = _dataset(400, 150, 0.06, seed=5)
    unset, named = EASEScorer(), EASEScorer()
    unset.train(ds, TrainingOptions(environment={}))
    named.train(ds, TrainingOptions(environment={"LK_EASE_SOLVER": "torch"}))
    assert np.array_equal(_bits(unset.weights), _bits(named.weights))
    dev = unset._device_weights()
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(unset.weights))
    for bad in ("scipy", "magic"):
        with pytest.raises(ValueError):
            EASEScorer().train(ds, TrainingOptions(environment={"LK_EASE_SOLVER": bad}))


# ---- lk_ease_score_panel ------------------------------------------------------------------------

def _histories(rng, n_items, n_queries):
    "empty, single, with -1, all -1, lengths 1 .. 9 (the unrolled loop's tails), long; then random"
    rows = [np.zeros(0, np.int32), np.array([n_items - 1], np.int32),
            np.array([2, -1, 0, -1], np.int32), np.array([-1, -1], np.int32)]
    rows += [rng.choice(n_items, min(l, n_items), replace=False).astype(np.int32)
             for l in range(1, 10)]
    rows.append(rng.permutation(n_items)[:min(n_items, 200)].astype(np.int32))
    while len(rows) < n_queries:
        rows.append(rng.choice(n_items, int(rng.integers(0, 12)), replace=False).astype(np.int32))
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, np.concatenate(rows).astype(np.int32), rows


@pytest.mark.parametrize("n_items", [33, 257, 1031])
def test_score_panel_bits_flags_and_window(gpu, rng, n_items):
    import torch

    from lkpy_amd import _device as D

    w = rng.standard_normal((n_items, n_items)).astype(np.float32)
    dw = torch.from_numpy(w).to(gpu)
    ptr, idx, rows = _histories(rng, n_items, 40)
    dptr, didx = torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)
    base = D.ease_score_batch(dptr, didx, dw).cpu().numpy()
    # the sequential float32 sum in history order, -1 adding nothing
    for q in (2, 8, 13):
        acc = np.zeros(n_items, np.float32)
        for it in rows[q]:
            if it >= 0:
                acc = acc + w[it]
        assert np.array_equal(_bits(base[q]), _bits(acc))
    plain = D.ease_score_panel(dptr, didx, dw).cpu().numpy()
    assert np.array_equal(_bits(plain), _bits(base))
    assert not plain[0].any() and not plain[3].any()  # no known item, no flag: zeros

    own = np.zeros((len(rows), n_items), bool)
    for q, r in enumerate(rows):
        own[q, r[r >= 0]] = True
    empty = ~own.any(axis=1)
    assert empty[0] and empty[3] and not empty[2]
    struck = D.ease_score_panel(dptr, didx, dw, strike_history=True).cpu().numpy()
    assert np.isnan(struck[own]).all() and np.array_equal(_bits(struck[~own]), _bits(base[~own]))
    nan_e = D.ease_score_panel(dptr, didx, dw, nan_empty=True).cpu().numpy()
    assert np.isnan(nan_e[empty]).all() and np.array_equal(_bits(nan_e[~empty]), _bits(base[~empty]))
    both = D.ease_score_panel(dptr, didx, dw, strike_history=True, nan_empty=True).cpu().numpy()
    assert np.isnan(both[empty]).all() and np.isnan(both[own]).all()
    keep = ~own & ~empty[:, None]
    assert np.array_equal(_bits(both[keep]), _bits(base[keep]))
    # a window of the rows
    part = D.ease_score_panel(dptr, didx, dw, rows=(5, 23), strike_history=True,
                              nan_empty=True).cpu().numpy()
    assert part.shape == (18, n_items)
    assert np.array_equal(_bits(part), _bits(both[5:23]))
    assert tuple(D.ease_score_panel(dptr, didx, dw, rows=(7, 7)).shape) == (0, n_items)


def test_score_panel_more_queries_than_a_grid_dimension(gpu, rng):
    import torch

    from lkpy_amd import _device as D

    n_items, n_queries = 33, 65539
    w = rng.standard_normal((n_items, n_items)).astype(np.float32)
    dw = torch.from_numpy(w).to(gpu)
    lens = rng.integers(0, 6, n_queries)
    ptr = np.zeros(n_queries + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = rng.integers(-1, n_items, int(ptr[-1])).astype(np.int32)
    dptr, didx = torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)
    got = D.ease_score_panel(dptr, didx, dw)
    want = D.ease_score_batch(dptr, didx, dw)  # (in calls of at most 65 535 queries)
    assert tuple(got.shape) == (n_queries, n_items)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert got[-1].cpu().numpy().any() or lens[-1] == 0


# ---- the component ------------------------------------------------------------------------------

class _Setup:
    def __init__(self):
        from lkpy_amd.data import Dataset, Vocabulary
        from lkpy_amd.knn import EASEScorer
        from lkpy_amd.pipeline import topn_pipeline

        base = _dataset(300, 260, 0.05, seed=17)
        self.lonely = int(base.users.ids().max()) + 1  # a known user without any item
        users = Vocabulary(np.append(base.users.ids(), self.lonely), "user")
        self.ds = Dataset(users, base.items, base._rows, base._cols, dict(base._attrs))
        self.ds.item_attrs["protected"] = np.random.default_rng(20).random(self.ds.item_count) < 0.2
        self.scorer = EASEScorer(regularization=2.0)
        self.pipe = topn_pipeline(self.scorer)
        self.pipe.train(self.ds)
        self.lookup = self.pipe.node("history-lookup").component
        uids = base.users.ids()
        self.users = [int(uids[i]) for i in np.linspace(0, len(uids) - 1, 50).astype(int)]
        assert len(set(self.users)) == 50


@pytest.fixture(scope="module")
def setup(gpu):
    return _Setup()


def _loop_forbidden(monkeypatch):
    from lkpy_amd import batch

    def never(*a, **k):
        raise AssertionError("the per-user loop was entered")

    monkeypatch.setattr(batch, "_recommend_loop", never)


def test_unique_histories_ascend(setup):
    from lkpy_amd._queries import pack_histories
    from lkpy_amd.data import ItemList, RecQuery

    ids = setup.ds.items.ids()
    q = RecQuery(user_items=ItemList(item_ids=np.array([ids[9], ids[2], 987654, ids[9], ids[4]])))
    ptr, idx, _ = pack_histories([q], setup.scorer.items, unknown="drop", unique=True)
    assert idx.tolist() == [2, 4, 9] and ptr.tolist() == [0, 3]


def test_batch_recommend_vs_per_user_pipeline(gpu, setup, monkeypatch):
    from lkpy_amd import batch

    s = setup
    loop = batch._recommend_loop(s.pipe, s.users + [s.lonely, -5], N_TOP)
    _loop_forbidden(monkeypatch)
    got = batch.recommend(s.pipe, s.users + [s.lonely, -5], N_TOP)
    assert len(got.lookup(s.lonely)) == 0 and len(loop.lookup(s.lonely)) == 0  # no known item
    assert len(got.lookup(-5)) == 0
    listed = 0
    for u in s.users:
        g, one = got.lookup(u), loop.lookup(u)
        hist = s.ds.user_row(u).numbers(vocabulary=s.ds.items)
        gi = np.asarray(g.numbers(vocabulary=s.scorer.items))
        assert len(gi) == N_TOP == len(np.unique(gi))
        assert not np.isin(gi, hist).any()  # history is excluded
        assert np.array_equal(gi, one.numbers(vocabulary=s.scorer.items)), u
        assert np.array_equal(_bits(g.scores()), _bits(one.scores())), u
        listed += len(gi)
    assert listed == 50 * N_TOP


def test_recommend_batch_front_ends_panels_and_pickle(gpu, setup):
    from lkpy_amd import _device as D
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.knn import EASEScorer

    s = setup
    scorer, lookup = s.scorer, s.lookup
    n_items = len(scorer.items)
    everyone = s.users + [s.lonely, -5]
    gi, gs = scorer.recommend_batch(lookup.batch(everyone), N_TOP)
    assert gi.shape == gs.shape == (52, N_TOP) and gi.dtype == np.int32
    assert (gi[-2:] == -1).all() and np.isnan(gs[-2:]).all() and (gi[:-2] >= 0).all()
    # a list of queries gives the same arrays as the HistoryBatch
    queries = [lookup(RecQuery.create(u)) for u in everyone]
    li, ls = scorer.recommend_batch(queries, N_TOP)
    assert np.array_equal(gi, li) and np.array_equal(_bits(gs), _bits(ls))
    # a batch split by a small PANEL_BYTES: the same bits as one panel
    assert scorer._panel_rows() >= 52
    old = EASEScorer.PANEL_BYTES
    try:
        EASEScorer.PANEL_BYTES = 4 * n_items * 7  # 52 queries = 7 panels of 7 and one of 3
        assert scorer._panel_rows() == 7
        pi, ps = scorer.recommend_batch(lookup.batch(everyone), N_TOP)
        qi, qs = scorer.recommend_batch(queries, N_TOP)
    finally:
        EASEScorer.PANEL_BYTES = old
    for i, v in ((pi, ps), (qi, qs)):
        assert np.array_equal(i, gi) and np.array_equal(_bits(v), _bits(gs))

    # dense_scores_batch: panel, valid, ascending known-item exclusion CSR
    some = s.users[:6] + [s.lonely, -5]
    for q in (lookup.batch(some), [lookup(RecQuery.create(u)) for u in some]):
        panel, valid, excl = scorer.dense_scores_batch(q)
        assert tuple(panel.shape) == (8, n_items) and list(valid) == [True] * 6 + [False] * 2
        host = panel.cpu().numpy()
        assert np.isnan(host[6:]).all() and not np.isnan(host[:6]).any()
        eptr, eidx = excl.indptr.cpu().numpy(), excl.indices.cpu().numpy()
        for r, u in enumerate(some[:6]):
            hist = np.sort(s.ds.user_row(u).numbers(vocabulary=s.ds.items))
            assert np.array_equal(eidx[eptr[r]:eptr[r + 1]], hist)
            # score_batch / __call__ give the panel's bits
            one = scorer(lookup(RecQuery.create(u)), ItemList(item_ids=s.ds.items.ids()))
            assert np.array_equal(_bits(one.scores()), _bits(host[r]))
        assert eptr[6] == eptr[8]
    # n = None ranks every candidate; exclude_history=False lists the history as well
    ni, ns = scorer.recommend_batch(lookup.batch(some), None)
    ai, _as = scorer.recommend_batch(lookup.batch(some), None, exclude_history=False)
    assert ni.shape == ai.shape == (8, n_items)
    idx = D.argtopn(panel, -1)
    assert np.array_equal(idx.cpu().numpy(), ai)
    for r, u in enumerate(some[:6]):
        hist = s.ds.user_row(u).numbers(vocabulary=s.ds.items)
        cand = n_items - len(hist)
        assert (ni[r, :cand] >= 0).all() and (ni[r, cand:] == -1).all()
        assert np.isnan(ns[r, cand:]).all() and (np.diff(ns[r, :cand]) <= 0).all()
        assert not np.isin(ni[r, :cand], hist).any()
        assert np.array_equal(_bits(host[r][ni[r, :cand]]), _bits(ns[r, :cand]))
        assert np.array_equal(np.sort(ai[r]), np.arange(n_items))
        assert np.array_equal(ni[r, :N_TOP], gi[r])
    assert (ni[6:] == -1).all()

    # a pickle round trip keeps host state only and still scores the same bits
    clone = pickle.loads(pickle.dumps(scorer))
    assert "_dev" not in clone.__dict__ and clone.is_trained()
    ci, cs = clone.recommend_batch(lookup.batch(everyone), N_TOP)
    assert np.array_equal(ci, gi) and np.array_equal(_bits(cs), _bits(gs))
    one = clone(queries[3], ItemList(item_ids=s.ds.items.ids()))
    assert np.array_equal(_bits(one.scores()),
                          _bits(scorer(queries[3], ItemList(item_ids=s.ds.items.ids())).scores()))


def test_stochastic_ranker_and_samples_take_the_panels(gpu, setup, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    s = setup
    p = Pipeline()
    p.nodes = {k: v for k, v in s.pipe.nodes.items() if k != "ranker"}
    p.aliases, p.default = dict(s.pipe.aliases), s.pipe.default
    p.add_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                    items="scorer", n="n", query="history-lookup")
    _loop_forbidden(monkeypatch)
    calls = []
    orig = p.run
    monkeypatch.setattr(p, "run", lambda *a, **k: (calls.append(a), orig(*a, **k))[1])
    users = s.users[:12]
    got = batch.recommend(p, users, N_TOP)
    many = batch.recommend_samples(p, users, N_TOP, 3)
    assert not calls, "the stochastic ranker must take the scorer's panels"
    assert many.key_fields == ("user_id", "sample") and len(many) == 36
    for u in users:
        own = s.ds.user_row(u).ids()
        for il in [got.lookup(u)] + [many.lookup(u, k) for k in range(3)]:
            assert len(il) == N_TOP and len(set(il.ids())) == N_TOP
            assert not np.isin(il.ids(), own).any()
        assert np.array_equal(got.lookup(u).ids(), many.lookup(u, 0).ids())


def test_fair_rerank_depth_takes_the_panels(gpu, setup, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.reranking import FAIRReranker

    s = setup
    both = Pipeline(s.pipe.name)
    both.nodes = dict(s.pipe.nodes)
    both.aliases, both.default = dict(s.pipe.aliases), s.pipe.default
    rr = FAIRReranker(n=N_TOP)
    rr.train(s.ds)
    both.add_reranker(rr)
    _loop_forbidden(monkeypatch)
    users = s.users[:20]
    deep = batch.recommend(both, users, N_TOP, rerank_depth=60)
    d_i, d_s = s.scorer.recommend_batch(s.lookup.batch(np.asarray(users)), 60)
    w_i, w_s = rr.rerank_batch(d_i, d_s, N_TOP)
    for r, u in enumerate(users):
        keep = w_i[r] >= 0
        assert keep.sum() == N_TOP
        assert np.array_equal(deep.lookup(u).numbers(vocabulary=s.scorer.items), w_i[r][keep])
        assert np.array_equal(_bits(deep.lookup(u).scores()), _bits(w_s[r][keep]))
        assert np.isin(w_i[r][keep], d_i[r]).all()
