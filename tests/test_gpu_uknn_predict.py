"""GPU: ``batch.predict`` for user-kNN pipelines as whole batches on the device
(csrc/uknn_predict.hip).  ``lk_uknn_score_pairs`` against the oracle's restatement of
src/accel/knn/user_score.rs fed the downloaded similarities; ``batch.predict`` against the
per-query composition it replaces (``batch._predict_loop``: history lookup, ``UserKNNScorer``,
``FallbackScorer`` over ``BiasScorer``); the reference's golden predictions; and the device caches
after a retrain.  Scores are compared as float32 bit patterns, NaN positions equal."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"

N_USERS, N_ITEMS, N_QUERIES = 200, 26, 65
UNRATED, SINGLE = 24, 25
THR = float(np.float32(1.0e-6))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_scores(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))


# ---- a. the kernel against the oracle -------------------------------------------------------------


class _Case:
    """200 users x 24 items at density 0.5 (columns of ~100 raters: two 64-entry chunks, and an
    accumulator that turns into a heap), item 0 at density 0.9 (three chunks, and a column longer
    than the 128 slots LDS holds: only then does ``max_nbrs = 128`` get the workspace slabs), item
    24 unrated, item 25 rated by one user; 65 queries drawn from the training rows with 0 .. 12
    targets each."""

    def __init__(self, gpu, oracle, explicit):
        import torch

        from lkpy_amd import _device as D

        rng = np.random.default_rng(20)
        dense = np.zeros((N_USERS, N_ITEMS), dtype=np.float32)
        mask = rng.random((N_USERS, 24)) < 0.5
        mask[:, 0] = rng.random(N_USERS) < 0.9
        dense[:, :24] = np.where(mask, rng.integers(1, 11, (N_USERS, 24)) * 0.5, 0)
        dense[17, SINGLE] = 4.0
        rmat = sps.csr_array(dense)
        rmat.sort_indices()
        if not explicit:
            rmat = sps.csr_array((np.ones_like(rmat.data), rmat.indices, rmat.indptr), rmat.shape)
        cols = np.diff(rmat.tocsc().indptr)
        assert cols[UNRATED] == 0 and cols[SINGLE] == 1 and cols[:24].min() > 64
        assert cols[0] > 128 and cols[1:24].max() < 128
        self.explicit = explicit
        uv, ur, _means = oracle.uknn_prepare(rmat, explicit)
        uv.sort_indices()
        self.ur = ur
        self.max_col = int(cols.max())
        vectors = D.DeviceCSR.from_arrays(uv.indptr, uv.indices, uv.data, uv.shape, gpu)
        ratings = D.DeviceCSR.from_host(ur.indptr, ur.indices, ur.data if explicit else None,
                                        ur.shape, gpu)
        self.ratings_t = D.csr_transpose(ratings, with_values=explicit)
        # the queries: training rows (their own users), histories = the raw rows
        users = rng.choice(N_USERS, N_QUERIES, replace=False)
        users[0] = 17  # (the single rater of item 25 asks, too)
        raw = sps.csr_array(dense)
        raw.sort_indices()
        h_ptr = np.zeros(N_QUERIES + 1, np.int64)
        np.cumsum(np.diff(raw.indptr)[users], out=h_ptr[1:])
        take = np.concatenate([np.arange(raw.indptr[u], raw.indptr[u + 1]) for u in users])
        h_items = raw.indices[take].astype(np.int32)
        h_rates = raw.data[take].astype(np.float32)
        centres = np.array([h_rates[h_ptr[q]:h_ptr[q + 1]].mean() for q in range(N_QUERIES)],
                           dtype=np.float32)
        hist = D.DeviceCSR.from_arrays(h_ptr, h_items, h_rates if explicit else None,
                                       (N_QUERIES, N_ITEMS), gpu)
        self.centre = torch.from_numpy(centres).to(gpu) if explicit else None
        self.offset = centres if explicit else np.zeros(N_QUERIES, np.float32)
        self.users = users
        self.self_user = torch.from_numpy(users.astype(np.int32)).to(gpu)
        x = D.uknn_query_panel(hist, self.centre)
        self.sims = D.csr_rows_dot(vectors, x)  # [queries x users], the self entries NOT zeroed
        self.S = self.sims.cpu().numpy()
        # the existing user-major panel (self entry +0.0) holds the same bits elsewhere
        self.panel = D.uknn_sims_panel(vectors, x, self.self_user, ld=N_QUERIES + 7)
        panel = self.panel.cpu().numpy()[:, :N_QUERIES]
        zeroed = self.S.copy()
        zeroed[np.arange(N_QUERIES), users] = 0.0
        assert np.array_equal(_bits(panel.T), _bits(zeroed))
        assert (self.S[np.arange(N_QUERIES), users] > 0.5).all()  # (they would pass)
        self.S0 = zeroed  # what the reference's neighbour list is drawn from
        # the targets: 0 .. 12 per query
        lists = []
        for q in range(N_QUERIES):
            n = int(rng.integers(0, 13))
            lists.append(rng.integers(0, N_ITEMS, n).astype(np.int32))
        lists[1] = np.zeros(0, np.int32)  # an empty list
        lists[2] = np.array([3, 7, 3, UNRATED, 3], np.int32)  # a repeated target
        lists[3] = np.array([5, -1, SINGLE, -1], np.int32)  # unknown items
        own = h_items[h_ptr[4]:h_ptr[5]]
        lists[4] = own[:12].copy()  # the query's own items
        lists[0] = np.array([SINGLE, UNRATED, 0], np.int32)  # the only rater is the query itself
        lists[64] = np.arange(12, dtype=np.int32)  # the query past the first 64
        self.t_ptr = np.zeros(N_QUERIES + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=self.t_ptr[1:])
        self.t_items = np.concatenate(lists)
        self.d_ptr = torch.from_numpy(self.t_ptr).to(gpu)
        self.d_items = torch.from_numpy(self.t_items).to(gpu)
        self._want = {}
        # per target entry: the passing raters its cell is offered (on the CPU)
        csc = ur.tocsc()
        q_of = np.repeat(np.arange(N_QUERIES), np.diff(self.t_ptr))
        self.held = np.array([
            0 if i < 0 else int((self.S0[q, csc.indices[csc.indptr[i]:csc.indptr[i + 1]]]
                                 >= np.float32(THR)).sum())
            for q, i in zip(q_of, self.t_items)])

    def want(self, oracle, max_nbrs, min_nbrs, S=None):
        "the oracle's scores of the target entries, per query, computed once per parameter pair"
        key = (max_nbrs, min_nbrs)
        if S is None and key in self._want:
            return self._want[key]
        S0 = self.S0 if S is None else S
        out = np.full(len(self.t_items), np.nan, dtype=np.float32)
        for q in range(N_QUERIES):
            lo, hi = self.t_ptr[q], self.t_ptr[q + 1]
            tgt = self.t_items[lo:hi]
            known = tgt >= 0
            if not known.any():
                continue
            nbrs = np.flatnonzero(S0[q] >= np.float32(THR))  # ascending user number; NaN fails
            sc = oracle.uknn_score(self.ur, nbrs, S0[q][nbrs], tgt[known], max_nbrs, min_nbrs,
                                   self.explicit)
            res = out[lo:hi]
            res[known] = sc + np.float32(self.offset[q]) if self.explicit else sc
        if S is None:
            self._want[key] = out
        return out

    def score(self, max_nbrs, min_nbrs, sims=None, **kw):
        from lkpy_amd import _device as D

        return D.uknn_score_pairs(self.ratings_t, self.sims if sims is None else sims,
                                  self.d_ptr, self.d_items, THR, max_nbrs, min_nbrs, self.centre,
                                  self_user=self.self_user, max_col=self.max_col, **kw)


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    made = {}

    def get(explicit):
        if explicit not in made:
            made[explicit] = _Case(gpu, oracle, explicit)
        return made[explicit]

    return get


def test_lds_limit_is_the_parametrised_boundary(gpu):
    from lkpy_amd import _device as D

    assert D.uknn_pairs_lds_max_nbrs() == 127


@pytest.mark.parametrize("max_nbrs,min_nbrs", [(1, 1), (3, 2), (20, 1), (127, 1), (128, 1)])
@pytest.mark.parametrize("explicit", [True, False])
def test_score_pairs_vs_oracle(gpu, oracle, cases, explicit, max_nbrs, min_nbrs):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    c = cases(explicit)
    lib = _native.load()
    # the accumulators of 127 live in LDS, those of 128 in the workspace slabs
    assert c.max_col > 128
    wb = lib.lk_uknn_score_pairs_workspace_bytes(max_nbrs, c.max_col)
    assert (wb > 0) == (max_nbrs > D.uknn_pairs_lds_max_nbrs())
    want = c.want(oracle, max_nbrs, min_nbrs)
    got = c.score(max_nbrs, min_nbrs).cpu().numpy()
    _same_scores(got, want)
    assert (~np.isnan(want)).sum() > 200
    # the cases this test is about are present
    if max_nbrs <= 20:
        assert c.held.max() > max_nbrs  # vector -> heap transition and evictions
    assert (c.held >= min_nbrs).any() and (c.held < min_nbrs).any()
    unknown = c.t_items < 0
    assert unknown.sum() == 2 and np.isnan(got[unknown]).all()
    assert np.isnan(got[c.t_items == UNRATED]).all()
    lo = c.t_ptr[0]
    assert np.isnan(got[lo])  # item 25's only rater is the query's own user: never passes
    lo = c.t_ptr[2]
    assert _bits(got[lo]) == _bits(got[lo + 2]) == _bits(got[lo + 4])  # the repeated target
    assert not np.isnan(got[c.t_ptr[4]:c.t_ptr[5]]).all()  # own items are scored like any other
    assert not np.isnan(got[c.t_ptr[64]:c.t_ptr[65]]).all()
    # the same bits again (no atomics), and with the entry range given
    again = c.score(max_nbrs, min_nbrs, entries=(0, len(c.t_items))).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got))
    # the user-major panel of lk_uknn_sims_panel (a wider leading dimension): the same cells
    major = c.score(max_nbrs, min_nbrs, sims=c.panel, user_major=True).cpu().numpy()
    assert np.array_equal(_bits(major), _bits(got))


def test_score_pairs_edges(gpu, oracle, cases):
    import torch

    from lkpy_amd import _device as D

    c = cases(True)
    base = c.score(20, 1).cpu().numpy()
    # a NaN similarity is ignored (user.py:206: the comparison fails)
    S = c.S0.copy()
    q = 5
    nbrs = np.flatnonzero(S[q] >= np.float32(THR))
    assert len(nbrs) > 3 and c.t_ptr[q + 1] > c.t_ptr[q]
    sims = c.sims.clone()
    for u in nbrs[:3]:
        sims[q, int(u)] = float("nan")
        S[q, u] = np.nan
    got = c.score(20, 1, sims=sims).cpu().numpy()
    _same_scores(got, c.want(oracle, 20, 1, S=S))
    rest = np.ones(len(base), bool)
    rest[c.t_ptr[q]:c.t_ptr[q + 1]] = False
    assert np.array_equal(_bits(got[rest]), _bits(base[rest]))
    # a step of the queries: a slice of the offsets, absolute entry numbers, the rest untouched
    out = torch.full((len(c.t_items),), 7.0, dtype=torch.float32, device=gpu)
    lo, hi = int(c.t_ptr[60]), int(c.t_ptr[65])
    ret = D.uknn_score_pairs(c.ratings_t, c.sims[60:].contiguous(), c.d_ptr[60:], c.d_items, THR,
                             20, 1, c.centre[60:], self_user=c.self_user[60:],
                             max_col=c.max_col, out=out, entries=(lo, hi))
    assert ret is out
    part = out.cpu().numpy()
    assert (part[:lo] == 7.0).all() and np.array_equal(_bits(part[lo:]), _bits(base[lo:]))
    # without self_user the own user's similarity counts: item 25's single rater scores it
    free = D.uknn_score_pairs(c.ratings_t, c.sims, c.d_ptr, c.d_items, THR, 20, 1, c.centre,
                              max_col=c.max_col).cpu().numpy()
    assert not np.isnan(free[c.t_ptr[0]])
    # zero queries / zero entries: clean returns; bad parameters raise
    none = D.uknn_score_pairs(c.ratings_t, c.sims[:0], c.d_ptr[:1], c.d_items[:0], THR, 20, 1,
                              max_col=c.max_col)
    assert tuple(none.shape) == (0,)
    with pytest.raises(Exception):
        c.score(0, 1)


# ---- b. the component against the per-query path ---------------------------------------------------


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _pairs(ds, n_users, seed=9):
    """``n_users`` users evenly over the dataset plus an unknown one, 5 .. 30 test items each, some
    item ids outside the vocabulary, one user with an empty list; every list carries a field"""
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(seed)
    uids = ds.users.ids()
    users = [int(uids[i]) for i in np.linspace(0, len(uids) - 1, n_users - 1).astype(int)]
    users.insert(7, 999_999)  # the unknown user
    items = ds.items.ids()
    pairs = {}
    for k, u in enumerate(users):
        ids = rng.choice(items, int(rng.integers(5, 31)), replace=False)
        if k % 6 == 0:
            ids[rng.integers(0, len(ids))] = 10**9 + k  # not in the vocabulary
        if k == 3:
            ids = ids[:0]
        pairs[u] = ItemList(item_ids=ids, rating=rng.integers(1, 11, len(ids)).astype(np.float32))
    return pairs


class _Setup:
    def __init__(self, ds, fallback=True, **config):
        from lkpy_amd.knn import UserKNNScorer
        from lkpy_amd.pipeline import predict_pipeline

        self.ds = ds
        self.pipe = predict_pipeline(UserKNNScorer(**config), fallback=fallback)
        self.pipe.train(ds)
        self.fallback = fallback
        self.pairs = _pairs(ds, 80)
        self._want = None

    def want(self):
        "the per-query composition (the parent's path for this pipeline), computed once"
        from lkpy_amd import batch

        if self._want is None:
            self._want = batch._predict_loop(self.pipe, self.pairs)
        return self._want


@pytest.fixture(scope="module")
def setups(gpu, ml_ds):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Setup(ml_ds, **{
                "explicit": dict(k=20),
                "nofallback": dict(k=20, min_nbrs=2, fallback=False),
                "implicit": dict(k=20, feedback="implicit")}[name])
        return made[name]

    return get


def _assert_same_lists(got, want, fallback):
    "key order, ids, field sets, score bits, is_fallback; no nbr_counts anywhere"
    assert [k.user_id for k in got.keys()] == [k.user_id for k in want.keys()]
    scored = fell = 0
    for (k, g), (_, w) in zip(got, want):
        assert np.array_equal(g.ids(), w.ids()), k
        assert list(g._fields) == list(w._fields), (k, list(g._fields), list(w._fields))
        assert "nbr_counts" not in g._fields and ("is_fallback" in g._fields) == fallback
        gs, ws = np.asarray(g.scores()), np.asarray(w.scores())
        assert np.array_equal(np.isnan(gs), np.isnan(ws)), k
        ok = ~np.isnan(ws)
        assert np.array_equal(_bits(gs[ok]), _bits(ws[ok])), k
        for f in w._fields:
            if f != "score":
                assert np.array_equal(g.field(f), w.field(f)), (k, f)
        if fallback:
            fell += int(np.asarray(w.field("is_fallback")).sum())
        scored += int(ok.sum())
    return scored, fell


def _no_loop(monkeypatch):
    from lkpy_amd import batch

    def boom(*_a, **_k):
        raise AssertionError("batch.predict fell back to the per-query loop")

    monkeypatch.setattr(batch, "_predict_loop", boom)


@pytest.mark.parametrize("name", ["explicit", "nofallback", "implicit"])
def test_predict_equals_the_per_query_path(setups, monkeypatch, name):
    from lkpy_amd import batch

    s = setups(name)
    want = s.want()
    _no_loop(monkeypatch)
    got = batch.predict(s.pipe, s.pairs)
    scored, fell = _assert_same_lists(got, want, s.fallback)
    total = sum(len(il) for il in s.pairs.values())
    assert 0 < scored <= total
    if s.fallback:
        assert 0 < fell < total  # both the primary and the fallback answer somewhere
    else:
        assert scored < total  # NaN where the scorer cannot answer
    assert len(got.lookup(999_999)) == len(s.pairs[999_999])
    u_empty = next(u for u, il in s.pairs.items() if len(il) == 0)
    assert len(got.lookup(u_empty)) == 0
    # bits do not depend on the batch size
    _assert_same_lists(batch.predict(s.pipe, s.pairs, batch_size=32), want, s.fallback)


def test_predict_bits_do_not_depend_on_the_panel_step(setups, monkeypatch):
    """``_panel_rows`` has a floor of 64 queries, so three steps need more than 128 queries: this
    case alone uses 140 users (64 + 64 + 12)."""
    from lkpy_amd import batch
    from lkpy_amd.knn import UserKNNScorer

    s = setups("explicit")
    pairs = _pairs(s.ds, 140, seed=10)
    want = batch._predict_loop(s.pipe, pairs)
    _no_loop(monkeypatch)
    whole = batch.predict(s.pipe, pairs)
    monkeypatch.setattr(UserKNNScorer, "PANEL_BYTES", 1)
    scorer = s.pipe.node("scorer").component
    assert scorer._panel_rows() == 64 and len(pairs) > 2 * 64
    steps = batch.predict(s.pipe, pairs)
    _assert_same_lists(whole, want, True)
    _assert_same_lists(steps, want, True)


def test_predict_takes_frames_and_collections(setups, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemListCollection

    s = setups("explicit")
    want = s.want()
    _no_loop(monkeypatch)
    ilc = ItemListCollection.from_dict(s.pairs, key=("user_id",))
    _assert_same_lists(batch.predict(s.pipe, ilc), want, True)
    df = ilc.to_df()
    got = batch.predict(s.pipe, df)
    # (a frame has no rows for the user with the empty list)
    keep = [(k, w) for k, w in want if len(w)]
    assert [k.user_id for k in got.keys()] == [k.user_id for k, _ in keep]
    for (k, g), (_, w) in zip(got, keep):
        assert np.array_equal(g.ids(), w.ids()) and list(g._fields) == list(w._fields)
        _same_scores(g.scores(), w.scores())
        assert np.array_equal(g.field("is_fallback"), w.field("is_fallback"))


# ---- c. golden ------------------------------------------------------------------------------------


def test_golden_predictions_through_batch_predict(gpu, ml_ds, monkeypatch):
    "user-user-preds.csv with the configuration and tolerance of test_user_knn_component_golden"
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import predict_pipeline

    pipe = predict_pipeline(UserKNNScorer(k=30, min_sim=1.0e-6), fallback=False)
    pipe.train(ml_ds)
    known = pd.read_csv(GOLDEN / "user-user-preds.csv")
    groups = list(known.groupby("user_id"))
    _no_loop(monkeypatch)
    res = batch.predict(pipe, {int(u): ItemList(g.item_id.values) for u, g in groups})
    got = np.concatenate([res.lookup(int(u)).scores() for u, _ in groups])
    exp = np.concatenate([g.prediction.values for _, g in groups])
    assert not np.any(np.isnan(got) & ~np.isnan(exp))
    err = np.abs(got - exp)
    err = err[~np.isnan(err)]
    assert len(err) > 0
    assert err.max() < 0.01 and np.median(err) < 1e-5, (err.max(), np.median(err))


def test_uknn_explicit_toml(gpu, ml_ds, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "uknn-explicit.toml")
    assert isinstance(pipe.node("scorer").component, UserKNNScorer)
    pipe.train(ml_ds)
    parts = batch._batched_predict_parts(pipe)
    assert parts is not None and isinstance(parts[2], BiasScorer)
    pairs = _pairs(ml_ds, 24, seed=12)
    want = batch._predict_loop(pipe, pairs)
    _no_loop(monkeypatch)
    scored, fell = _assert_same_lists(batch.predict(pipe, pairs), want, True)
    assert scored > fell > 0


# ---- d. retrain -----------------------------------------------------------------------------------


def test_predict_follows_a_retrain(gpu, ml_ds, monkeypatch):
    "the device caches (model, transposed ratings, centres, lookup matrix) follow ``Pipeline.train``"
    from lkpy_amd import batch
    from lkpy_amd.data import Dataset, ItemList
    from lkpy_amd.knn import UserKNNScorer
    from lkpy_amd.pipeline import predict_pipeline

    rng = np.random.default_rng(5)
    items = ml_ds.items.ids()
    n_users, nnz = 300, 20_000
    pop = 1.0 / (rng.permutation(len(items)) + 10.0)
    cells = np.unique(rng.integers(0, n_users, nnz) * len(items) +
                      rng.choice(len(items), nnz, p=pop / pop.sum()))
    syn = Dataset.from_arrays(cells // len(items) + 5_000_000, items[cells % len(items)],
                              rng.integers(1, 11, len(cells)) * 0.5, all_item_ids=items)
    assert syn.items == ml_ds.items and syn.users != ml_ds.users

    def check(pipe, ds, seed):
        r = np.random.default_rng(seed)
        users = [int(u) for u in ds.users.ids()[::12]] + [-5]
        pairs = {u: ItemList(np.concatenate([r.choice(items, 20, replace=False), [10**9]]))
                 for u in users}
        want = batch._predict_loop(pipe, pairs)
        with monkeypatch.context() as m:
            _no_loop(m)
            got = batch.predict(pipe, pairs)
        scored, fell = _assert_same_lists(got, want, True)
        assert scored > fell > 0

    pipe = predict_pipeline(UserKNNScorer(k=20))
    pipe.train(ml_ds)
    check(pipe, ml_ds, 1)
    pipe.train(syn)  # every component retrained on the second dataset
    check(pipe, syn, 2)
    # the lookup alone back on the first data: the user vocabularies differ -- the loop again
    pipe.node("history-lookup").component.train(ml_ds)
    assert batch._batched_predict_parts(pipe) is None
