"""GPU parity: user-kNN for whole panels of queries (csrc/uknn_recommend.hip).  The score panel
against the oracle's restatement of src/accel/knn/user_score.rs fed the downloaded similarities,
the similarity panel against ``csr_rows_dot``, the query panel against the host-built dense rows,
and ``batch.recommend`` against one ``pipe.run`` per user of the same pipeline."""
import pickle
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"

N_USERS, N_ITEMS, N_QUERIES = 150, 90, 70
ISOLATED, CONSTANT, TWIN_A, TWIN_B = 149, 148, 10, 11
THR = float(np.float32(1.0e-6))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _synthetic(rng):
    """150 users x 90 items, ratings from {0.5 .. 5.0}: item 0 unrated, item 1 rated by exactly
    64 users, item 2 by 140 (three chunks of 64), items 3 .. 87 at ~15 %; user 149 alone on items
    88 and 89; user 148 rates everything 3.0; users 10 and 11 have equal rows (tied similarities)."""
    dense = np.zeros((N_USERS, N_ITEMS), dtype=np.float32)
    val = lambda shape: (rng.integers(1, 11, shape) * 0.5).astype(np.float32)  # noqa: E731
    mask = rng.random((ISOLATED, 85)) < 0.15
    dense[:ISOLATED, 3:88] = np.where(mask, val((ISOLATED, 85)), 0)
    pool = np.array([u for u in range(ISOLATED) if u not in (TWIN_A, TWIN_B)])
    dense[rng.choice(pool, 64, replace=False), 1] = val(64)  # (neither twin)
    dense[rng.choice(pool, 138, replace=False), 2] = val(138)
    dense[TWIN_A, 2] = 3.5  # (both twins: 140)
    dense[TWIN_B] = dense[TWIN_A]
    dense[CONSTANT, 3:6] = 3.0
    dense[CONSTANT] = np.where(dense[CONSTANT] > 0, 3.0, 0)
    dense[ISOLATED, 88:90] = (4.5, 2.0)
    rmat = sps.csr_array(dense)
    rmat.sort_indices()
    cols = np.diff(rmat.tocsc().indptr)
    assert cols[0] == 0 and cols[1] == 64 and cols[2] > 128 and cols[88] == cols[89] == 1
    return rmat


def _queries(rmat, rng, explicit):
    """70 queries (two lane blocks, the second partial): 69 training users with their own rows as
    history, then one without a user whose history has an unknown item and a repeated one.
    Returns (host offsets, items, ratings, centres f32, self users, host-built X [items x 70])."""
    others = [u for u in rng.permutation(N_USERS) if u not in (ISOLATED, CONSTANT, TWIN_A, TWIN_B)]
    users = [ISOLATED, CONSTANT, TWIN_A, TWIN_B] + [int(u) for u in others[:N_QUERIES - 5]]
    ptr, items, rates, selves = [0], [], [], []
    for u in users:
        s, e = rmat.indptr[u], rmat.indptr[u + 1]
        items.append(rmat.indices[s:e].astype(np.int32))
        rates.append(rmat.data[s:e].astype(np.float32))
        selves.append(u)
    items.append(np.array([5, -1, 7, 5, 9], dtype=np.int32))
    rates.append(np.array([4.0, 3.0, 2.5, 1.0, 5.0], dtype=np.float32))
    selves.append(-1)
    for it in items:
        ptr.append(ptr[-1] + len(it))
    centres = np.array([r.mean() for r in rates], dtype=np.float32)
    X = np.zeros((N_ITEMS, len(items)), dtype=np.float32)
    for q, (nos, urv) in enumerate(zip(items, rates)):
        row = np.zeros(N_ITEMS, dtype=np.float32)  # user.py:296-304, as UserKNNScorer._user_data
        ok = nos >= 0
        row[nos[ok]] = (urv[ok] - float(centres[q])) if explicit else 1.0
        X[:, q] = row
    assert len(items) == N_QUERIES
    return (np.array(ptr, dtype=np.int64), np.concatenate(items), np.concatenate(rates), centres,
            np.array(selves, dtype=np.int32), X)


class _Case:
    "the synthetic model and queries of one feedback mode on the device, with the sims downloaded"

    def __init__(self, gpu, oracle, rng, explicit):
        import torch

        from lkpy_amd import _device as D

        raw = rmat = _synthetic(rng)
        if not explicit:
            rmat = sps.csr_array((np.ones_like(raw.data), raw.indices, raw.indptr), raw.shape)
        self.explicit = explicit
        uv, ur, _means = oracle.uknn_prepare(rmat, explicit)
        uv.sort_indices()
        self.ur = ur
        self.vectors = D.DeviceCSR.from_arrays(uv.indptr, uv.indices, uv.data, uv.shape, gpu)
        ratings = D.DeviceCSR.from_host(ur.indptr, ur.indices, ur.data if explicit else None,
                                        ur.shape, gpu)
        self.ratings_t = D.csr_transpose(ratings, with_values=explicit)
        self.max_col = int(np.diff(ur.tocsc().indptr).max())
        ptr, items, rates, centres, selves, X = _queries(raw, rng, explicit)
        self.ptr, self.items, self.X, self.selves = ptr, items, X, selves
        self.hist = D.DeviceCSR.from_arrays(ptr, items, rates if explicit else None,
                                            (N_QUERIES, N_ITEMS), gpu)
        self.centre = torch.from_numpy(centres).to(gpu)
        self.offset = centres if explicit else np.zeros(N_QUERIES, np.float32)
        self.self_user = torch.from_numpy(selves).to(gpu)
        self.x = D.uknn_query_panel(self.hist, self.centre if explicit else None)
        self.sims = D.uknn_sims_panel(self.vectors, self.x, self.self_user)
        self.S = self.sims.cpu().numpy()  # [users x queries]: the oracle's neighbours come from it
        self._want = {}
        self._census = None

    def census(self):
        """On the CPU, from the oracle's inputs: per cell the passing raters it is offered
        [items x queries], and the number of cells in which two of them have bit-equal sims."""
        if self._census is None:
            passing = self.S >= np.float32(THR)  # [users x queries]
            csc = self.ur.tocsc()
            held = np.zeros((N_ITEMS, N_QUERIES), dtype=np.int64)
            tied = 0
            for i in range(N_ITEMS):
                raters = csc.indices[csc.indptr[i]:csc.indptr[i + 1]]
                held[i] = passing[raters].sum(axis=0)
                for q in range(N_QUERIES):
                    s = self.S[raters, q][passing[raters, q]]
                    tied += int(len(np.unique(s)) < len(s))
            self._census = held, tied
        return self._census

    def want(self, oracle, max_nbrs, min_nbrs):
        "the oracle's panel for these parameters, computed once"
        key = (max_nbrs, min_nbrs)
        if key not in self._want:
            out = np.empty((N_QUERIES, N_ITEMS), dtype=np.float32)
            everything = np.arange(N_ITEMS, dtype=np.int32)
            for q in range(N_QUERIES):
                nbrs = np.flatnonzero(self.S[:, q] >= np.float32(THR))  # ascending user number
                sc = oracle.uknn_score(self.ur, nbrs, self.S[nbrs, q], everything, max_nbrs,
                                       min_nbrs, self.explicit)
                out[q] = sc + np.float32(self.offset[q]) if self.explicit else sc
            self._want[key] = out
        return self._want[key]

    def score(self, max_nbrs, min_nbrs, **kw):
        from lkpy_amd import _device as D

        return D.uknn_score_panel(self.ratings_t, self.sims, N_QUERIES, THR, max_nbrs, min_nbrs,
                                  self.centre if self.explicit else None, max_col=self.max_col,
                                  **kw)


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    made = {}

    def get(explicit, rng):
        "(the first test to ask builds the case, from its own fresh ``rng``)"
        if explicit not in made:
            made[explicit] = _Case(gpu, oracle, rng, explicit)
        return made[explicit]

    return get


@pytest.mark.parametrize("explicit", [True, False])
def test_query_panel_and_sims_panel(gpu, cases, rng, explicit):
    import torch

    from lkpy_amd import _device as D

    c = cases(explicit, rng)
    # X = the host-built dense rows: last occurrence of the repeated item, the -1 skipped
    x = c.x.cpu().numpy()
    assert x.shape == (N_ITEMS, N_QUERIES) and np.array_equal(_bits(x), _bits(c.X))
    assert x[5, -1] == (np.float32(1.0) - np.float32(c.offset[-1]) if explicit else 1.0)
    wide = D.uknn_query_panel(c.hist, c.centre if explicit else None, ld=80).cpu().numpy()
    assert np.array_equal(_bits(wide[:, :N_QUERIES]), _bits(c.X)) and not wide[:, N_QUERIES:].any()
    part = D.uknn_query_panel(c.hist, c.centre if explicit else None, rows=(64, 70))
    assert np.array_equal(_bits(part.cpu().numpy()), _bits(c.X[:, 64:]))
    # the user-major sims = csr_rows_dot's bits, transposed; the self entry +0.0
    flat = D.csr_rows_dot(c.vectors, c.x).cpu().numpy()  # [queries x users]
    want = flat.T.copy()
    for q, u in enumerate(c.selves):
        if u >= 0:
            want[u, q] = 0.0
    assert np.array_equal(_bits(c.S), _bits(want))
    own = [(u, q) for q, u in enumerate(c.selves) if u >= 0]
    assert all(_bits(c.S[u, q]) == 0 for u, q in own)
    assert np.any(flat[[q for _, q in own], [u for u, _ in own]] > 0.5)  # (they were not zero)
    padded = D.uknn_sims_panel(c.vectors, c.x, c.self_user, ld=96).cpu().numpy()
    assert padded.shape == (N_USERS, 96) and np.array_equal(_bits(padded[:, :N_QUERIES]), _bits(want))
    # zero queries: clean returns
    empty = D.DeviceCSR.from_arrays(np.zeros(1, np.int64), np.zeros(0, np.int32), None,
                                    (0, N_ITEMS), gpu)
    assert tuple(D.uknn_query_panel(empty, None).shape) == (N_ITEMS, 0)
    none = torch.empty((N_ITEMS, 0), dtype=torch.float32, device=gpu)
    assert tuple(D.uknn_sims_panel(c.vectors, none).shape) == (N_USERS, 0)


@pytest.mark.parametrize("max_nbrs,min_nbrs", [(1, 1), (3, 2), (30, 1), (300, 1)])
@pytest.mark.parametrize("explicit", [True, False])
def test_score_panel_vs_oracle(gpu, oracle, cases, rng, explicit, max_nbrs, min_nbrs):
    import torch

    from lkpy_amd import _device as D

    c = cases(explicit, rng)
    # -- on the CPU, from the oracle's inputs: the cases this test is about are present --------
    held, tied = c.census()
    csc = c.ur.tocsc()
    if max_nbrs < N_USERS:
        assert held.max() > max_nbrs  # vector -> heap transition and evictions
    else:  # no cell can fill it: this is the case of the global-slab accumulators
        assert min(max_nbrs, c.max_col) > D.uknn_lds_max_nbrs()
    assert tied > 0
    want = c.want(oracle, max_nbrs, min_nbrs)
    assert not np.isnan(want).all() and np.isnan(want).any()

    # -- the panel: the oracle's NaN pattern and bits ------------------------------------------
    got = c.score(max_nbrs, min_nbrs).cpu().numpy()
    assert got.shape == (N_QUERIES, N_ITEMS)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))
    assert np.isnan(got[0]).all()  # the isolated user: no neighbour
    if explicit:
        assert np.isnan(got[1]).all()  # constant ratings: the centred vector is all zero
    assert np.isnan(got[:, 0]).all()  # the item nobody rated
    # without the item order = with it (heaviest column first)
    order = np.argsort(-np.diff(csc.indptr), kind="stable").astype(np.int32)
    again = c.score(max_nbrs, min_nbrs, item_order=torch.from_numpy(order).to(gpu)).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got))

    # -- struck cells are NaN only with the flag; a wider leading dimension is honoured --------
    out = torch.full((N_QUERIES, N_ITEMS + 7), 7.0, dtype=torch.float32, device=gpu)
    ret = c.score(max_nbrs, min_nbrs, hist=c.hist, strike_history=True, out=out)
    assert ret is out
    struck = out.cpu().numpy()
    assert (struck[:, N_ITEMS:] == 7.0).all()
    struck = struck[:, :N_ITEMS]
    own = np.zeros((N_QUERIES, N_ITEMS), dtype=bool)
    for q in range(N_QUERIES):
        nos = c.items[c.ptr[q]:c.ptr[q + 1]]
        own[q, nos[nos >= 0]] = True
    assert (~np.isnan(got[own])).any()  # (the flag has something to strike)
    assert np.isnan(struck[own]).all()
    assert np.array_equal(_bits(struck[~own]), _bits(got[~own]))


def test_score_panel_edges(gpu, cases, rng):
    import torch

    from lkpy_amd import _device as D

    c = cases(True, rng)
    # nan_empty: the row of a query without a known history item
    ptr = c.ptr.copy()
    items = c.items.copy()
    items[ptr[3]:ptr[4]] = -1
    hist = D.DeviceCSR.from_arrays(ptr, items, None, (N_QUERIES, N_ITEMS), gpu)
    base = c.score(30, 1).cpu().numpy()
    got = c.score(30, 1, hist=hist, nan_empty=True).cpu().numpy()
    assert not np.isnan(base[3]).all() and np.isnan(got[3]).all()
    rest = np.arange(N_QUERIES) != 3
    assert np.array_equal(_bits(got[rest]), _bits(base[rest]))
    # a panel of some rows of the histories
    part = D.uknn_score_panel(c.ratings_t, c.sims[:, 64:].contiguous(), 6, THR, 30, 1,
                              c.centre[64:70], hist=c.hist, rows=(64, 70), strike_history=True,
                              max_col=c.max_col).cpu().numpy()
    full = c.score(30, 1, hist=c.hist, strike_history=True).cpu().numpy()
    assert np.array_equal(_bits(part), _bits(full[64:]))
    # zero queries, zero items: clean returns
    none = torch.empty((N_USERS, 0), dtype=torch.float32, device=gpu)
    assert tuple(D.uknn_score_panel(c.ratings_t, none, 0, THR, 30, 1, max_col=c.max_col).shape) \
        == (0, N_ITEMS)
    no_items = D.DeviceCSR(torch.zeros(1, dtype=torch.int64, device=gpu),
                           torch.zeros(0, dtype=torch.int32, device=gpu), None, (0, N_USERS), None)
    assert tuple(D.uknn_score_panel(no_items, c.sims, N_QUERIES, THR, 30, 1, max_col=0).shape) \
        == (N_QUERIES, 0)
    with pytest.raises(Exception):
        D.uknn_score_panel(c.ratings_t, c.sims, N_QUERIES, THR, 0, 1, max_col=c.max_col)


# ---- the component on ml_small ------------------------------------------------------------------

N_TOP = 10


class _Setup:
    def __init__(self, **config):
        from lkpy_amd.data import load_movielens_npz
        from lkpy_amd.knn import UserKNNScorer
        from lkpy_amd.pipeline import topn_pipeline

        self.ds = load_movielens_npz(GOLDEN / "ml_small.npz")
        self.scorer = UserKNNScorer(**config)
        self.pipe = topn_pipeline(self.scorer)
        self.pipe.train(self.ds)
        self.lookup = self.pipe.node("history-lookup").component
        uids = self.ds.users.ids()
        self.users = [int(uids[i]) for i in np.linspace(0, len(uids) - 1, 64).astype(int)]
        assert len(set(self.users)) == 64
        self._runs = {}

    def run(self, u):
        "the per-user pipeline's list (today's score_batch + TopNRanker), computed once"
        if u not in self._runs:
            self._runs[u] = self.pipe.run("recommender", query=u, n=N_TOP)
        return self._runs[u]


@pytest.fixture(scope="module")
def setups(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Setup(**{"k30": dict(k=30, min_sim=1.0e-6),
                                   "k3": dict(k=3, min_nbrs=2),
                                   "implicit": dict(k=30, feedback="implicit")}[name])
        return made[name]

    return get


def _no_pipe_run(pipe, call):
    calls = []
    orig = pipe.run
    pipe.run = lambda *a, **k: (calls.append(a), orig(*a, **k))[1]
    try:
        out = call()
    finally:
        pipe.run = orig
    assert not calls, "batch.recommend must not fall back to one pipeline run per user"
    return out


def _compare_with_pipeline(s, users):
    from lkpy_amd import batch

    got = _no_pipe_run(s.pipe, lambda: batch.recommend(s.pipe, users + [-7], N_TOP))
    assert len(got.lookup(-7)) == 0  # the unknown user: nothing listed
    panel, valid, _excl = s.scorer.dense_scores_batch(s.lookup.batch(users))
    panel = panel.cpu().numpy()
    assert valid.all()
    ties = listed = 0
    for r, u in enumerate(users):
        g, one = got.lookup(u), s.run(u)
        hist = s.ds.user_row(u).numbers(vocabulary=s.ds.items)
        gi = np.asarray(g.numbers(vocabulary=s.scorer.items))
        oi = np.asarray(one.numbers(vocabulary=s.scorer.items))
        gs, os_ = np.asarray(g.scores(), np.float32), np.asarray(one.scores(), np.float32)
        assert len(gi) == len(oi) and len(np.unique(gi)) == len(gi)
        assert not np.isin(gi, hist).any()  # no history item is listed
        assert np.array_equal(_bits(gs), _bits(os_)), u  # position by position
        assert np.array_equal(_bits(panel[r][gi]), _bits(gs))  # an item carries its own score
        assert np.array_equal(_bits(panel[r][oi]), _bits(os_))
        ties += int(not np.array_equal(gi, oi))
        listed += len(gi)
    assert listed > 0
    print(f"\n{len(users)} users: lists differing among bit-equal scores: {ties}")
    return got


@pytest.mark.parametrize("name", ["k30", "k3"])
def test_batch_recommend_vs_pipeline(gpu, setups, name):
    s = setups(name)
    _compare_with_pipeline(s, s.users)


def test_batch_recommend_implicit(gpu, setups):
    s = setups("implicit")
    _compare_with_pipeline(s, s.users[::4])


def test_recommend_batch_front_ends_and_panels(gpu, setups):
    from lkpy_amd import _device as D
    from lkpy_amd.data import RecQuery
    from lkpy_amd.knn import UserKNNScorer

    s = setups("k30")
    scorer, lookup = s.scorer, s.lookup
    n_items = len(scorer.items)
    with_unknown = s.users + [-7]
    gi, gs = scorer.recommend_batch(lookup.batch(with_unknown), N_TOP)
    assert gi.shape == gs.shape == (65, N_TOP) and gi.dtype == np.int32
    # HistoryBatch input and list-of-queries input: identical arrays
    li, ls = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in with_unknown], N_TOP)
    assert np.array_equal(gi, li) and np.array_equal(_bits(gs), _bits(ls))
    assert (gi[-1] == -1).all() and np.isnan(gs[-1]).all()  # the unknown user
    assert (gi[:-1] >= 0).any()
    # three panels, the last partial: 65 queries in panels of 64 need a floor below 64 ...
    assert scorer._panel_rows() >= 64
    old = UserKNNScorer.PANEL_BYTES
    many = (s.users * 3)[:150] + [-7]  # ... so 151 queries: 64 + 64 + 23
    try:
        whole = scorer.recommend_batch(lookup.batch(many), N_TOP)
        UserKNNScorer.PANEL_BYTES = 1
        assert scorer._panel_rows() == 64
        pi, ps = scorer.recommend_batch(lookup.batch(many), N_TOP)
        qi, qs = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in many], N_TOP)
    finally:
        UserKNNScorer.PANEL_BYTES = old
    for i, v in ((pi, ps), (qi, qs)):
        assert np.array_equal(i, whole[0]) and np.array_equal(_bits(v), _bits(whole[1]))
    assert np.array_equal(pi[:64], gi[:64]) and np.array_equal(_bits(ps[:64]), _bits(gs[:64]))

    some = with_unknown[:7] + [-7]
    batch8 = lookup.batch(some)
    # dense_scores_batch = recommend_batch's scores through argtopn
    ai, _as = scorer.recommend_batch(batch8, None, exclude_history=False)
    ei, _es = scorer.recommend_batch(batch8, 50)
    # n = None ranks every scorable candidate in order; a larger n than that pads
    panel, valid, excl = scorer.dense_scores_batch(batch8)
    assert tuple(panel.shape) == (8, n_items) and valid.tolist() == [True] * 7 + [False]
    own = [len(s.ds.user_row(u)) for u in some[:7]]
    assert np.array_equal(np.diff(excl.indptr.cpu().numpy()), own + [0])
    idx = D.argtopn(panel, -1)
    sc = D.take_scores(panel, idx).cpu().numpy()
    assert np.array_equal(idx.cpu().numpy(), ai) and np.array_equal(_bits(sc), _bits(_as))
    host = panel.cpu().numpy()
    assert np.isnan(host[-1]).all()
    # exclude_history=False lists history items where they score (and only there)
    seen = 0
    for r, u in enumerate(some[:7]):
        hist = s.ds.user_row(u).numbers(vocabulary=s.ds.items)
        scored = hist[~np.isnan(host[r][hist])]
        assert np.isin(scored, ai[r]).all() and not np.isin(ei[r][ei[r] >= 0], hist).any()
        assert int(np.isin(ai[r][ai[r] >= 0], hist).sum()) == len(scored)
        seen += len(scored)
    assert seen > 0
    ni, ns = scorer.recommend_batch(batch8, None)
    assert ni.shape == (8, n_items)
    for r, u in enumerate(some[:7]):
        hist = s.ds.user_row(u).numbers(vocabulary=s.ds.items)
        row = host[r].copy()
        row[hist] = np.nan
        scorable = int((~np.isnan(row)).sum())
        assert 0 < scorable < n_items
        assert (ni[r, :scorable] >= 0).all() and (ni[r, scorable:] == -1).all()  # padded
        assert np.isnan(ns[r, scorable:]).all()
        assert np.array_equal(_bits(row[ni[r, :scorable]]), _bits(ns[r, :scorable]))
        assert (np.diff(ns[r, :scorable]) <= 0).all()  # in order
        assert np.array_equal(ni[r, :50], ei[r]) or \
            np.array_equal(_bits(ns[r, :50]), _bits(_es[r]))
    assert (ni[-1] == -1).all()
    wide_i, wide_s = scorer.recommend_batch(batch8, n_items + 5)
    assert wide_i.shape == (8, n_items + 5) and (wide_i[:, n_items:] == -1).all()
    assert np.array_equal(wide_i[:, :n_items], ni) and np.isnan(wide_s[:, n_items:]).all()

    # a pickle round trip keeps host state only and recommends the same bits
    clone = pickle.loads(pickle.dumps(scorer))
    assert "_dev" not in clone.__dict__ and clone.is_trained()
    ci, cs = clone.recommend_batch([lookup(RecQuery.create(u)) for u in with_unknown], N_TOP)
    assert np.array_equal(ci, gi) and np.array_equal(_bits(cs), _bits(gs))
    ci, cs = clone.recommend_batch(lookup.batch(with_unknown), N_TOP)
    assert np.array_equal(ci, gi) and np.array_equal(_bits(cs), _bits(gs))


def test_stored_vector_branch_and_missing_ratings(gpu, setups):
    "a known user WITHOUT history is scored from the stored vector, like score_batch"
    from lkpy_amd.basic import UserTrainingHistoryLookup
    from lkpy_amd.data import Dataset, ItemList, RecQuery

    s = setups("k30")
    u = s.users[5]
    gi, gs = s.scorer.recommend_batch([RecQuery(user_id=u), RecQuery(user_id=-5)], N_TOP,
                                      exclude_history=False)
    want = s.scorer(RecQuery(user_id=u), ItemList(item_ids=s.ds.items.ids())).top_n(N_TOP)
    assert np.array_equal(_bits(gs[0]), _bits(np.asarray(want.scores(), np.float32)))
    assert (gi[1] == -1).all() and np.isnan(gs[1]).all()
    # an explicit scorer over a lookup without ratings raises, like ItemKNNScorer
    bare = Dataset(s.ds.users, s.ds.items, s.ds._rows, s.ds._cols, {})
    lookup = UserTrainingHistoryLookup()
    lookup.train(bare)
    with pytest.raises(RuntimeError, match="must have ratings"):
        s.scorer.recommend_batch(lookup.batch(s.users[:3]), N_TOP)


def test_stochastic_ranker_takes_the_panels(gpu, setups):
    from lkpy_amd import batch
    from lkpy_amd.stochastic import StochasticTopNRanker

    s = setups("k30")
    pipe = s.pipe
    node = pipe.nodes["ranker"]
    kept = node.component, dict(node.wiring)
    users = s.users[:12]
    try:
        pipe.replace_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                               query="history-lookup")
        got = _no_pipe_run(pipe, lambda: batch.recommend(pipe, users, N_TOP))
        many = _no_pipe_run(pipe, lambda: batch.recommend_samples(pipe, users, N_TOP, 3))
    finally:
        node.component, node.wiring = kept
    assert many.key_fields == ("user_id", "sample") and len(many) == 36
    for u in users:
        own = s.ds.user_row(u).ids()
        for il in [got.lookup(u)] + [many.lookup(u, k) for k in range(3)]:
            assert len(il) == N_TOP and len(set(il.ids())) == N_TOP
            assert not np.isin(il.ids(), own).any()
        assert np.array_equal(got.lookup(u).ids(), many.lookup(u, 0).ids())
