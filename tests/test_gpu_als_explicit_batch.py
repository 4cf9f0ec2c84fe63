"""GPU: ``BiasedMFScorer`` for whole batches -- csrc/bmf_batch.hip against the NumPy restatement
(tests/als_explicit_batch_restatement.py) bit for bit, and ``batch.recommend`` / ``batch.predict``
/ ``dense_scores_batch`` on ml-latest-small with ``als-explicit.toml`` against the per-query
pipeline they replace."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import als_explicit_batch_restatement as R
from test_gpu_als import RTOL, _rel

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
N_TOP = 10


def _dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- kernel (1): lk_bmf_residual_rows ----------------------------------------------------------

ROW_LENGTHS = (0, 1, 7, 8, 9, 128, 129, 8193)  # the pairwise-sum tree's edges


@pytest.fixture(scope="module")
def rows_case():
    "a training matrix with one row per length, item-sorted, half-star ratings; item biases"
    rng = np.random.default_rng(17)
    n_items = 9000
    indptr = np.zeros(len(ROW_LENGTHS) + 1, dtype=np.int64)
    np.cumsum(ROW_LENGTHS, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(n_items, n, replace=False))
                              for n in ROW_LENGTHS]).astype(np.int32)
    ratings = (rng.integers(1, 11, len(indices)) / 2).astype(np.float32)
    item_biases = rng.normal(0, 0.4, n_items).astype(np.float32)
    mu = 3.5430217
    users = np.array([7, -1, 0, 1, 2, 3, 4, 5, 6, 7, -1, 3], dtype=np.int32)
    want = {}
    for damping in (0.0, 5.0):
        want[damping] = [R.residuals(ratings[indptr[u]:indptr[u + 1]],
                                     indices[indptr[u]:indptr[u + 1]], mu, item_biases, damping)
                         if u >= 0 else None for u in users]
    return SimpleNamespace(n_items=n_items, indptr=indptr, indices=indices, ratings=ratings,
                           item_biases=item_biases, mu=mu, users=users, want=want)


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("damping", [0.0, 5.0])
def test_residual_rows_equal_the_restatement(gpu, rows_case, is64, damping):
    from lkpy_amd import _device as D

    c = rows_case
    mat = D.DeviceCSR.from_arrays(c.indptr.astype(np.int64 if is64 else np.int32), c.indices,
                                  c.ratings, (len(ROW_LENGTHS), c.n_items), gpu)
    assert mat.is64 == is64
    csr, ub = D.bmf_residual_rows(mat, c.users, c.mu, _dev(c.item_biases, gpu), damping)
    ptr, idx, val = csr.indptr.cpu().numpy(), csr.indices.cpu().numpy(), csr.values.cpu().numpy()
    ub = ub.cpu().numpy()
    assert ptr.dtype == np.int64 and np.array_equal(ptr, csr.h_indptr) and ub.dtype == np.float64
    lens = [0 if u < 0 else ROW_LENGTHS[u] for u in c.users]
    assert np.array_equal(np.diff(ptr), lens) and len(idx) == len(val) == sum(lens)
    for q, w in enumerate(c.want[damping]):
        lo, hi = ptr[q], ptr[q + 1]
        if w is None:
            assert ub[q] == 0.0 and lo == hi
            continue
        nums, res, w_ub = w
        assert np.float64(ub[q]).tobytes() == np.float64(w_ub).tobytes(), (q, ub[q], w_ub)
        assert np.array_equal(idx[lo:hi], nums), q
        assert np.array_equal(R.bits(val[lo:hi]), R.bits(res)), q


# ---- kernels (2) and (3) on a synthetic panel ------------------------------------------------


def _panel_case(n_items, seed):
    rng = np.random.default_rng(seed)
    modes = np.array([R.FOLD, R.STORED, R.INVALID, R.FOLD, R.STORED, R.FOLD, R.STORED],
                     dtype=np.uint8)
    rows = len(modes)
    panel = rng.normal(0, 0.7, (rows, n_items)).astype(np.float32)
    panel[0, 0] = np.float32(1e-30)
    ub = rng.normal(0, 0.3, rows)  # float64 on a fold-in row
    ub[modes == R.STORED] = ub[modes == R.STORED].astype(np.float32)  # the model's float32
    ub[modes == R.INVALID] = 0.0
    item_biases = rng.normal(0, 0.4, n_items).astype(np.float32)
    return modes, panel, ub, item_biases, 3.5430217, rng


@pytest.mark.parametrize("n_items", [1, 63, 257, 1000, 2051])
def test_finish_panel_equals_the_restatement(gpu, n_items):
    from lkpy_amd import _device as D

    modes, panel, ub, item_biases, mu, rng = _panel_case(n_items, n_items)
    rows = len(modes)
    every = np.arange(n_items)
    want = np.stack([R.finish(panel[r], every, mu, item_biases, int(modes[r]), ub[r])
                     for r in range(rows)])
    got = D.bmf_finish_panel(_dev(panel, gpu), _dev(modes, gpu), _dev(ub, gpu), mu,
                             _dev(item_biases, gpu)).cpu().numpy()
    assert np.array_equal(R.bits(got), R.bits(want))
    assert np.isnan(got[2]).all() and not np.isnan(got[[0, 1, 3, 4, 5, 6]]).any()
    # strikes: the first item, the last item, both, an empty history, a few in the middle
    hist = [[0], [n_items - 1], [0, n_items - 1], [], sorted(set(rng.integers(0, n_items, 5))),
            [], [n_items // 2]]
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum([len(h) for h in hist], out=ptr[1:])
    items = np.concatenate([np.asarray(h, dtype=np.int32) for h in hist]).astype(np.int32)
    struck = want.copy()
    for r, h in enumerate(hist):
        struck[r, h] = np.nan
    got = D.bmf_finish_panel(_dev(panel, gpu), _dev(modes, gpu), _dev(ub, gpu), mu,
                             _dev(item_biases, gpu), _dev(ptr, gpu), _dev(items, gpu))
    assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(struck))


@pytest.mark.parametrize("n_items", [1, 63, 257, 1000])
def test_finish_pairs_equals_the_restatement(gpu, n_items):
    import torch

    from lkpy_amd import _device as D

    modes, panel, ub, item_biases, mu, rng = _panel_case(n_items, 100 + n_items)
    rows = len(modes)
    last = n_items - 1
    targets = [[0, last, -1, 0, 0], [], [last], [0, -1], list(rng.integers(0, n_items, 40)), [],
               [-1, last, last]]  # an empty list, unknown items, repeated targets
    ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum([len(t) for t in targets], out=ptr[1:])
    items = np.concatenate([np.asarray(t, dtype=np.int32) for t in targets]).astype(np.int32)
    want = np.concatenate([R.finish(panel[r][np.maximum(np.asarray(t, dtype=np.int64), 0)],
                                    np.asarray(t, dtype=np.int64), mu, item_biases,
                                    int(modes[r]), ub[r]) for r, t in enumerate(targets)])
    d_panel, d_modes, d_ub = _dev(panel, gpu), _dev(modes, gpu), _dev(ub, gpu)
    d_ptr, d_items, d_ib = _dev(ptr, gpu), _dev(items, gpu), _dev(item_biases, gpu)
    out = torch.full((len(items),), 7.0, dtype=torch.float32, device=gpu)
    D.bmf_finish_pairs(d_panel, d_modes, d_ub, mu, d_ib, d_ptr, d_items, 0, len(items), out)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(want))
    # by panels of rows, as the scorer steps: rows 2..4 alone write their own entries only
    out = torch.full((len(items),), 7.0, dtype=torch.float32, device=gpu)
    first, count = int(ptr[2]), int(ptr[5] - ptr[2])
    D.bmf_finish_pairs(d_panel[2:5].contiguous(), d_modes[2:5], d_ub[2:5], mu, d_ib, d_ptr[2:6],
                       d_items, first, count, out)
    got = out.cpu().numpy()
    assert np.array_equal(R.bits(got[first:first + count]), R.bits(want[first:first + count]))
    assert (got[:first] == 7.0).all() and (got[first + count:] == 7.0).all()


# ---- the pipeline on ml-latest-small ---------------------------------------------------------


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _train(ml_ds, user_embeddings, *, fallback=True):
    from lkpy_amd import als
    from lkpy_amd.pipeline import Pipeline, predict_pipeline
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "als-explicit.toml")
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, als.BiasedMFScorer)
    if not fallback:
        pipe = predict_pipeline(scorer, fallback=False)
    scorer.config.embedding_size = 20
    scorer.config.epochs = 4
    scorer.config.user_embeddings = user_embeddings
    pipe.train(ml_ds, TrainingOptions(rng=42))
    return pipe


@pytest.fixture(scope="module", params=[True, "prefer", False],
                ids=["default", "prefer", "no-user-embeddings"])
def setup(request, gpu, ml_ds):
    pipe = _train(ml_ds, request.param)
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    ids = ml_ds.users.ids()
    users = np.concatenate([ids[::7], [ids.max() + 5, ids.max() + 9]])  # + two unknown users
    return SimpleNamespace(pipe=pipe, scorer=scorer, lookup=lookup, users=users, ds=ml_ds,
                           mode=request.param)


def _forbid_the_loop(monkeypatch, pipe):
    def boom(*_a, **_k):
        raise AssertionError("pipe.run called: the per-query loop")

    monkeypatch.setattr(pipe, "run", boom)


def _collection_arrays(out, users, vocab, n):
    idx = np.full((len(users), n), -1, dtype=np.int32)
    sc = np.full((len(users), n), np.nan, dtype=np.float32)
    for r, u in enumerate(users.tolist()):
        il = out.lookup(u)
        idx[r, :len(il)] = il.numbers(vocabulary=vocab)
        sc[r, :len(il)] = il.scores()
    return idx, sc


def test_recommend_batch_equals_the_per_query_pipeline(setup):
    from lkpy_amd import batch
    from lkpy_amd.data import RecQuery

    s = setup
    queries = [s.lookup(RecQuery.create(u.item())) for u in s.users]
    li, ls = s.scorer.recommend_batch(queries, N_TOP)
    hi, hs = s.scorer.recommend_batch(s.lookup.batch(s.users), N_TOP)
    assert li.dtype == np.int32 and ls.dtype == np.float32 and li.shape == (len(s.users), N_TOP)
    assert np.array_equal(li, hi) and np.array_equal(R.bits(ls), R.bits(hs))
    bi, bs = _collection_arrays(batch.recommend(s.pipe, s.users, N_TOP), s.users,
                                s.scorer.items, N_TOP)
    assert np.array_equal(bi, hi) and np.array_equal(R.bits(bs), R.bits(hs))
    # the two unknown users: nothing to score; every known user: a full list without own items
    assert (hi[-2:] == -1).all() and np.isnan(hs[-2:]).all()
    assert (hi[:-2] >= 0).all() and not np.isnan(hs[:-2]).any()
    for r, u in enumerate(s.users[:-2].tolist()):
        own = s.ds.user_row(u).numbers(vocabulary=s.scorer.items)
        assert not np.isin(hi[r], own).any(), u
        assert len(set(hi[r].tolist())) == N_TOP and np.all(np.diff(hs[r]) <= 0)
    # the per-query pipeline: the same score bits (equal scores may list different items)
    for r in (0, len(s.users) // 2, len(s.users) - 3):
        one = s.pipe.run("recommender", query=s.users[r].item(), n=N_TOP)
        assert np.array_equal(R.bits(one.scores()), R.bits(hs[r])), r
    one = s.pipe.run("recommender", query=s.users[-1].item(), n=N_TOP)
    assert len(one) == 0 or np.isnan(one.scores()).all()
    # left on the device: the same arrays
    di, dsc = s.scorer.recommend_batch(s.lookup.batch(s.users), N_TOP, device_output=True)
    assert di.is_cuda and dsc.is_cuda
    assert np.array_equal(di.cpu().numpy(), hi)
    assert np.array_equal(R.bits(dsc.cpu().numpy()), R.bits(hs))
    # history kept: a user's own items may be listed, and scores are no lower
    ki, ks = s.scorer.recommend_batch(s.lookup.batch(s.users), N_TOP, exclude_history=False)
    assert np.all(ks[:-2, 0] >= hs[:-2, 0])


def test_recommend_batch_in_several_panels_and_every_candidate(setup):
    s = setup
    hb = s.lookup.batch(s.users)
    hi, hs = s.scorer.recommend_batch(hb, N_TOP)
    n_items = len(s.scorer.items)
    s.scorer.PANEL_BYTES = 4 * n_items * 13  # 13 rows a panel
    try:
        assert s.scorer._panel_rows() == 13 < len(s.users)
        pi, ps = s.scorer.recommend_batch(s.lookup.batch(s.users), N_TOP)
    finally:
        del s.scorer.PANEL_BYTES
    assert np.array_equal(pi, hi) and np.array_equal(R.bits(ps), R.bits(hs))
    # n = None / negative: every candidate, ranked
    few = s.lookup.batch(s.users[[0, 5, len(s.users) - 1]])
    ai, asc = s.scorer.recommend_batch(few, None)
    assert ai.shape == (3, n_items) and np.array_equal(ai[:, :N_TOP][:2], hi[[0, 5]])
    for r, u in enumerate(s.users[[0, 5]].tolist()):
        assert (ai[r] >= 0).sum() == n_items - len(s.ds.user_row(u))
    assert (ai[2] == -1).all() and np.isnan(asc[2]).all()


def test_batch_calls_run_without_the_per_query_loop(setup, monkeypatch):
    "fails on a scorer without the batched paths: ``batch.recommend`` / ``predict`` loop ``pipe.run``"
    from lkpy_amd import batch

    s = setup
    rng = np.random.default_rng(3)
    pairs = {u: rng.choice(s.ds.items.ids(), 5, replace=False) for u in s.users[:9].tolist()}
    _forbid_the_loop(monkeypatch, s.pipe)
    got = batch.recommend(s.pipe, s.users, N_TOP)
    assert len(got) == len(s.users) and len(got.lookup(s.users[0].item())) == N_TOP
    pred = batch.predict(s.pipe, pairs)
    assert type(pred._lists).__name__ == "_RaggedLists"  # the batched path
    assert len(pred) == 9 and all(len(il) == 5 for _k, il in pred)


def test_list_queries_mix_the_three_branches(setup):
    "a known user without history (stored row), a history without a user (fold-in), neither"
    from lkpy_amd.data import ItemList, RecQuery

    s = setup
    u0, u1 = s.users[0].item(), s.users[1].item()
    hist = s.ds.user_row(u1)
    bad = ItemList(item_ids=np.concatenate([hist.ids()[:6], [-5]]),  # an unknown item, a NaN
                   rating=np.concatenate([hist.field("rating")[:5], [np.nan, 4.0]])
                   .astype(np.float32))
    queries = [s.lookup(RecQuery.create(u0)), RecQuery(user_id=u1), RecQuery(user_items=hist),
               RecQuery(user_id=s.users[-1].item()), RecQuery(user_id=u0, user_items=bad)]
    every = ItemList.from_vocabulary(s.scorer.items)
    want = [np.asarray(s.scorer(q, every).scores(), dtype=np.float32) for q in queries]
    assert np.isnan(want[3]).all()
    assert np.isnan(want[2]).all() == (s.mode == "prefer")  # (no stored row to prefer: NaN)
    assert not np.isnan(want[0]).any() and not np.isnan(want[4]).any()
    assert np.isnan(want[1]).all() == (s.mode is False)  # (no stored rows kept)
    panel, valid, hcsr = s.scorer.dense_scores_batch(queries)
    got = panel.cpu().numpy()
    assert np.array_equal(valid, [not np.isnan(w).all() for w in want])
    for r in range(len(queries)):
        assert np.array_equal(R.bits(got[r]), R.bits(want[r])), r
    assert np.array_equal(np.diff(hcsr.h_indptr), [len(s.ds.user_row(u0)), 0, len(hist), 0, 6])
    # score_batch: ragged targets with an unknown item, a repeated one and an empty list
    ids = s.scorer.items.ids()
    lists = [ItemList(item_ids=np.array([ids[0], -3, ids[-1], ids[0]])), ItemList(item_ids=ids[:7]),
             ItemList(item_ids=ids[:0]), ItemList(item_ids=ids[5:9]), ItemList(item_ids=ids[::900])]
    scored = s.scorer.score_batch(queries, lists)
    for q, il, sc in zip(queries, lists, scored):
        assert np.array_equal(sc.ids(), il.ids())
        w = np.asarray(s.scorer(q, il).scores(), dtype=np.float32) if len(il) else np.zeros(0)
        assert np.array_equal(R.bits(sc.scores()), R.bits(w))


@pytest.mark.parametrize("fallback", [True, False], ids=["fallback", "no-fallback"])
def test_predict_equals_the_per_query_pipeline(setup, ml_ds, fallback, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import predict_pipeline

    s = setup
    pipe = s.pipe
    if not fallback:  # the same trained scorer and lookup, no fallback-predictor / merger
        pipe = predict_pipeline(s.scorer, fallback=False)
        pipe.node("history-lookup").component = s.lookup
    rng = np.random.default_rng(11)
    users = s.users[::3].tolist() + [s.users[-1].item()]  # (an unknown user among them)
    pairs = {u: ItemList(item_ids=rng.choice(ml_ds.items.ids(), 9, replace=False)) for u in users}
    pairs[users[0]] = ItemList(item_ids=np.concatenate([pairs[users[0]].ids(), [-7, 10**9]]))
    pairs[users[1]] = ItemList(item_ids=ml_ds.items.ids()[:0])  # an empty list
    want = {u: pipe.run("rating-predictor", query=u, items=il) for u, il in pairs.items()}
    for size in (16384, 7):  # one batch; several
        got = batch.predict(pipe, pairs, batch_size=size)
        assert type(got._lists).__name__ == "_RaggedLists"  # the batched path
        for u, w in want.items():
            g = got.lookup(u)
            assert np.array_equal(g.ids(), w.ids()), u
            assert list(g._fields) == list(w._fields), (u, list(g._fields), list(w._fields))
            assert g.scores().dtype == np.float32
            assert np.array_equal(R.bits(g.scores()), R.bits(w.scores())), u
            if fallback:
                assert np.array_equal(g.field("is_fallback"), w.field("is_fallback")), u
    fb = np.concatenate([w.field("is_fallback") for w in want.values()]) if fallback else None
    unknown = want[users[-1]].scores()
    if fallback:
        assert fb.any() and not fb.all() and not np.isnan(unknown).any()
    else:
        assert np.isnan(unknown).all() and np.isnan(want[users[0]].scores()[-2:]).all()


def test_dense_scores_and_the_stochastic_ranker(setup, monkeypatch):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    s = setup
    users = s.users[[0, 3, 8, len(s.users) - 1]]
    panel, valid, hist = s.scorer.dense_scores_batch(s.lookup.batch(users))
    got = panel.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (4, len(s.scorer.items))
    assert valid.tolist() == [True, True, True, False] and np.isnan(got[3]).all()
    every = ItemList.from_vocabulary(s.scorer.items)
    for r, u in enumerate(users[:3].tolist()):
        one = s.scorer(s.lookup(RecQuery.create(u)), every).scores()
        assert np.array_equal(R.bits(got[r]), R.bits(one)), u
    assert np.array_equal(np.diff(hist.h_indptr)[:3], [len(s.ds.user_row(u))
                                                       for u in users[:3].tolist()])
    p = Pipeline()
    p.nodes = {k: v for k, v in s.pipe.nodes.items() if k != "ranker"}
    p.aliases, p.default = dict(s.pipe.aliases), s.pipe.default
    p.add_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                    items="scorer", n="n", query="history-lookup")
    assert batch._has_panels(s.scorer, s.lookup)
    _forbid_the_loop(monkeypatch, p)
    out = batch.recommend(p, s.users[:12], N_TOP)
    for u in s.users[:12].tolist():
        il = out.lookup(u)
        assert len(il) == N_TOP and len(set(il.ids())) == N_TOP
        assert not np.isin(il.ids(), s.ds.user_row(u).ids()).any()


def test_fold_in_embeddings_of_a_batch(setup):
    "the batch's explicit half-epoch against ``_train_bias_row_cholesky`` restated in float64"
    from lkpy_amd import _device as D
    from lkpy_amd.basic import _damping

    s = setup
    users = s.users[:40]
    hb = s.lookup.batch(users)
    kept = s.scorer.config.user_embeddings
    if kept == "prefer":  # (the same model folds in once stored rows are no longer preferred)
        s.scorer.config.user_embeddings = True
    try:
        u, mode, _d_mode, ub, _hist, pending = s.scorer._batch_operands(hb)
        for plan in pending:
            plan.check_status()
        alone = np.stack([D.to_host_unpadded(
            s.scorer._batch_operands(s.lookup.batch(users[r:r + 1]))[0],
            s.scorer.config.embedding_size)[0] for r in (0, 7, 39)])
    finally:
        s.scorer.config.user_embeddings = kept
    k = s.scorer.config.embedding_size
    got = D.to_host_unpadded(u, k)
    ub = ub.cpu().numpy()
    assert (mode == R.FOLD).all()
    Q = s.scorer.item_embeddings.astype(np.float64)
    bias = s.scorer.bias
    want = np.zeros_like(got, dtype=np.float64)
    for r, uid in enumerate(users.tolist()):
        row = s.ds.user_row(uid)
        nums, res, w_ub = R.residuals(row.field("rating"), row.numbers(vocabulary=s.scorer.items),
                                      bias.global_bias, bias.item_biases,
                                      _damping(bias.damping, "user"))
        assert np.float64(ub[r]).tobytes() == np.float64(w_ub).tobytes()
        M = Q[nums]
        A = M.T @ M + np.eye(k) * (s.scorer.config.user_reg * len(nums))
        want[r] = np.linalg.solve(A, M.T @ res.astype(np.float64))
    assert _rel(got, want) < RTOL
    err = np.linalg.norm(got - want, axis=1)
    assert np.all(err <= 5 * RTOL * np.maximum(np.linalg.norm(want, axis=1), 1e-3))
    # a row solved inside the batch against the same row solved alone (reported)
    differ = [r for i, r in enumerate((0, 7, 39)) if not np.array_equal(alone[i], got[r])]
    print("rows whose batched solve differs in bits from the solve alone:", differ)


def test_retrained_lookup_serves_the_new_matrix(gpu, ml_ds):
    "retrain on other data: the batch reads the NEW training matrix, like the per-query path"
    from lkpy_amd import batch
    from lkpy_amd.data import Dataset, RecQuery
    from lkpy_amd.training import TrainingOptions

    pipe = _train(ml_ds, True)
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    users = ml_ds.users.ids()[::40]
    before = batch.recommend(pipe, users, N_TOP)  # (the first matrix is now resident)
    assert lookup.ratings_finite()
    keep = np.random.default_rng(9).random(len(ml_ds._rows)) < 0.6
    other = Dataset(ml_ds.users, ml_ds.items, ml_ds._rows[keep], ml_ds._cols[keep],
                    {"rating": ml_ds._attrs["rating"][keep]})
    pipe.train(other, TrainingOptions(rng=42))
    hb = lookup.batch(users)
    assert np.array_equal(hb.lengths, [len(other.user_row(u)) for u in users.tolist()])
    assert np.array_equal(np.diff(hb.csr(with_values=False).h_indptr), hb.lengths)
    bi, bs = _collection_arrays(batch.recommend(pipe, users, N_TOP), users, scorer.items, N_TOP)
    li, ls = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in users.tolist()], N_TOP)
    assert np.array_equal(bi, li) and np.array_equal(R.bits(bs), R.bits(ls))
    for r in (0, len(users) - 1):
        one = pipe.run("recommender", query=users[r].item(), n=N_TOP)
        assert np.array_equal(R.bits(one.scores()), R.bits(bs[r]))
        assert not np.isin(bi[r], other.user_row(users[r].item())
                           .numbers(vocabulary=scorer.items)).any()
    first = before.lookup(users[0].item())
    assert not np.array_equal(R.bits(first.scores()), R.bits(bs[0]))  # (another model)
