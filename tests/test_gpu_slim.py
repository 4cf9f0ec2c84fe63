"""
SLIM / fsSLIM on the device (csrc/slim.hip) against the NumPy restatement of the reference's
``compute_column`` (``tests/slim_restatement.py``; src/accel/slim/mod.rs:147-300).

Bar: the learned rows equal the restatement's index arrays and value BITS -- the soft threshold
and the stopping test are discontinuous, so no tolerance describes a reordered sum.  Scores equal
SciPy's ``x @ weights`` bit for bit; recommendation lists may differ from the per-user pipeline
only among items with identical score bits (counted and printed).
"""
import pickle
import threading
import time
from pathlib import Path

import numpy as np
import pyarrow as pa
import pytest
import scipy.sparse as sps

from slim_restatement import csr_pair, slim_rows

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
CONFIGS = [(1.0, 1.0, 100, None), (1.0, 1.0, 100, 500), (0.005, 0.01, 10, 100)]


def _device_pair(m, gpu, dtype=np.int32):
    import torch

    from lkpy_amd import _device as D

    ui_ptr, ui_idx, iu_ptr, iu_idx = m
    n_users, n_items = len(ui_ptr) - 1, len(iu_ptr) - 1

    def up(ptr, idx, shape):
        h = ptr.astype(dtype)
        return D.DeviceCSR(torch.from_numpy(h).to(gpu), torch.from_numpy(idx.copy()).to(gpu),
                           None, shape, h)

    return up(ui_ptr, ui_idx, (n_users, n_items)), up(iu_ptr, iu_idx, (n_items, n_users))


def _host(csr):
    return (csr.indptr.cpu().numpy(), csr.indices.cpu().numpy(), csr.values.cpu().numpy())


def _assert_rows_equal(got, want, what=""):
    gp, gi, gv = got
    wp, wi, wv = want
    assert np.array_equal(gp, wp), f"{what}: row lengths differ"
    assert np.array_equal(gi, wi), f"{what}: indices differ"
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), f"{what}: value bits differ"


@pytest.fixture(scope="module")
def ml_pair(ml_small):
    return csr_pair(sps.csr_array(ml_small["rmat"]))


@pytest.fixture(scope="module")
def ml_columns(ml_pair):
    "the 3 most-rated items, 40 sampled rated items (seeded), one unrated item"
    n_of = np.diff(ml_pair[2])
    rng = np.random.default_rng(20261016)
    rated = np.flatnonzero(n_of > 0)
    top = np.argsort(-n_of, kind="stable")[:3]
    sample = rng.choice(np.setdiff1d(rated, top), 40, replace=False)
    unrated = np.flatnonzero(n_of == 0)[:1]
    assert len(unrated) == 1
    return np.concatenate([top, sample, unrated]).astype(np.int32)


@pytest.fixture(scope="module")
def ml_restated(ml_pair, ml_columns):
    "config -> (rows, per-column info) of the restatement on the sampled columns"
    out = {}
    for cfg in CONFIGS:
        infos = []
        out[cfg] = (slim_rows(*ml_pair, ml_columns, *cfg, infos=infos), infos)
    return out


@pytest.mark.parametrize("cfg", CONFIGS, ids=["slim", "fsslim-500", "trainer-test"])
def test_kernel_equals_restatement_bit_for_bit(gpu, ml_small, ml_pair, ml_columns, ml_restated,
                                               cfg):
    from lkpy_amd import _device as D

    assert sps.csr_array(ml_small["rmat"]).shape == (671, 9125)
    l1, l2, iters, k = cfg
    ui, iu = _device_pair(ml_pair, gpu)
    stats = {}
    got = D.slim_train(ui, iu, l1, l2, iters, k, columns=ml_columns, stats=stats)
    want, infos = ml_restated[cfg]
    rounds = [i["rounds"] for i in infos]
    print(f"\n{cfg}: {int(want[0][-1])} weights on {len(ml_columns)} columns, rounds "
          f"{min(rounds)}..{max(rounds)}, largest active list {max(i['active'] for i in infos)}, "
          f"{sum(i['cut'] for i in infos)} columns cut; coordinate updates "
          f"{stats['coord_updates']}, residual entries {stats['resid_entries']}")
    _assert_rows_equal(_host(got), want, str(cfg))
    assert got.shape == (len(ml_columns), 9125)
    # the kernel counted what the restatement counted
    assert stats["rounds"] == sum(rounds)
    assert stats["coord_updates"] == sum(i["coord_updates"] for i in infos)
    assert stats["resid_entries"] == sum(i["resid_entries"] for i in infos)


def test_sample_exercises_both_exits_and_the_cut(ml_restated):
    "what the parity test relies on, asserted about its own inputs"
    early = capped = False
    for (l1, l2, iters, k), (_rows, infos) in ml_restated.items():
        early |= any(i["rounds"] < iters for i in infos)
        capped |= any(i["rounds"] == iters for i in infos)
    assert early, "no sampled column stops by the tolerance"
    assert capped, "no sampled column runs to max_iters"
    infos = ml_restated[CONFIGS[1]][1]
    assert any(i["cut"] for i in infos) and max(i["active"] for i in infos) > 500


def test_stable_cut_under_ties(gpu):
    from lkpy_amd import _device as D

    mat = sps.random_array((300, 120), density=0.08, rng=np.random.default_rng(42))
    mat.data[:] = 1.0
    m = csr_pair(mat)
    infos = []
    cols = np.arange(120, dtype=np.int32)
    want = slim_rows(*m, cols, 1.0, 1.0, 100, 10, infos=infos)
    n_cut = sum(i["cut"] for i in infos)
    n_tie = sum(i["tie_at_cut"] for i in infos)
    print(f"\n{n_cut} of 120 columns cut, {n_tie} with equal keys on both sides of the cut")
    assert n_cut > 100 and n_tie > 10  # the stable order matters on this input
    ui, iu = _device_pair(m, gpu)
    got = D.slim_train(ui, iu, 1.0, 1.0, 100, 10)  # columns=None: all 120
    assert got.shape == (120, 120)
    _assert_rows_equal(_host(got), want, "ties")
    # 64-bit offsets take the other instantiation: the same rows
    ui64, iu64 = _device_pair(m, gpu, np.int64)
    _assert_rows_equal(_host(D.slim_train(ui64, iu64, 1.0, 1.0, 100, 10)), want, "ties, i64")


def test_residuals_in_the_workspace_beyond_the_lds_bound(gpu):
    """More users than the LDS residual vector holds (4096): the wave's residuals live in its
    workspace slot.  5000 users x 80 items, fsSLIM cut at 20 and plain SLIM, every column."""
    from lkpy_amd import _device as D

    mat = sps.random_array((5000, 80), density=0.03, rng=np.random.default_rng(9))
    mat.data[:] = 1.0
    m = csr_pair(mat)
    ui, iu = _device_pair(m, gpu)
    cols = np.arange(80, dtype=np.int32)
    for cfg in [(0.5, 0.5, 30, 20), (1.0, 1.0, 100, None)]:
        _assert_rows_equal(_host(D.slim_train(ui, iu, *cfg)), slim_rows(*m, cols, *cfg), str(cfg))


def test_column_list(gpu, ml_pair, ml_columns):
    from lkpy_amd import _device as D

    ui, iu = _device_pair(ml_pair, gpu)
    big = _host(D.slim_train(ui, iu, 0.005, 0.01, 10, 100, columns=ml_columns))
    pick = [7, 0, 21]
    small = _host(D.slim_train(ui, iu, 0.005, 0.01, 10, 100, columns=ml_columns[pick]))
    for r, p in enumerate(pick):
        a = slice(big[0][p], big[0][p + 1])
        b = slice(small[0][r], small[0][r + 1])
        assert np.array_equal(big[1][a], small[1][b])
        assert np.array_equal(big[2][a].view(np.uint32), small[2][b].view(np.uint32))
    # several batches of columns (a staging budget of a few rows) give the same matrix
    old = D.SLIM_STAGE_BYTES
    try:
        D.SLIM_STAGE_BYTES = 8 * 100 * 16
        parts = _host(D.slim_train(ui, iu, 0.005, 0.01, 10, 100, columns=ml_columns))
    finally:
        D.SLIM_STAGE_BYTES = old
    _assert_rows_equal(parts, big, "batched")
    with pytest.raises(ValueError):
        D.slim_train(ui, iu, 1.0, 1.0, 10, None, columns=[9125])


def test_seam_train_slim_consumer_lines(gpu, ml_small, ml_pair, ml_columns, ml_restated):
    "tests/models/test_slim.py::test_slim_trainer of the reference + progress"
    from lkpy_amd import _accel
    from lkpy_amd.matrix import SparseRowArray
    from lkpy_amd.parallel import run_accel_task

    rmat = sps.csr_array(ml_small["rmat"])
    ui = SparseRowArray.from_scipy(rmat, values=False)
    iu = ui.transpose()
    n_items = rmat.shape[1]
    task = _accel.slim.train_slim(ui, iu, 0.005, 0.01, 10, 100)
    result = run_accel_task(task)
    assert task.current_progress() == (n_items, n_items)
    assert isinstance(result, list)
    result = pa.chunked_array(result).combine_chunks()
    assert pa.types.is_large_list(result.type)
    result = SparseRowArray.from_array(result)
    assert result.shape == (n_items, n_items)
    # the sampled rows of the full fit are the restatement's
    want = ml_restated[CONFIGS[2]][0]
    off = result.offsets.to_numpy()
    idx, val = result.indices.to_numpy(), result.values.to_numpy()
    for r, c in enumerate(ml_columns):
        a, b = slice(off[c], off[c + 1]), slice(want[0][r], want[0][r + 1])
        assert np.array_equal(idx[a], want[1][b])
        assert np.array_equal(val[a].view(np.uint32), want[2][b].view(np.uint32))


def test_cancel_reaches_the_running_trainer(gpu, ml_pair):
    from lkpy_amd import _accel
    from lkpy_amd import _device as D
    from lkpy_amd.matrix import SparseRowArray
    from lkpy_amd.parallel import run_accel_task

    ui, iu = _device_pair(ml_pair, gpu)
    # cancelled before the launch: no column starts, the call says so
    ctl = D.TaskCtl()
    ctl.cancel()
    with pytest.raises(KeyboardInterrupt):
        D.slim_train(ui, iu, 1.0, 1.0, 100, None, ctl=ctl)
    done, total = ctl.progress()
    assert total == 9125 and done == 0

    # cancelled mid-flight through the attached control block
    ctl2 = D.TaskCtl()
    err = []

    def work():
        try:
            D.slim_train(ui, iu, 1.0, 1.0, 100, None, ctl=ctl2)
        except BaseException as e:  # noqa: BLE001
            err.append(e)

    th = threading.Thread(target=work)
    th.start()
    while th.is_alive() and ctl2.progress()[0] == 0:
        time.sleep(0.0002)
    ctl2.cancel()
    th.join()
    done, total = ctl2.progress()
    print(f"\ncancel mid-flight: stopped at {done} of {total} columns, error: {err!r}")
    # the race is real (the fit may finish first); when the cancel won, the call must say so
    if err:
        assert isinstance(err[0], KeyboardInterrupt) and done < total
    else:
        assert done == total

    # through the task protocol, like the similarity build's task: cancel() -> KeyboardInterrupt
    # inside, RuntimeError("accelerator task failed ...") from run_accel_task
    rmat = sps.csr_array((np.ones(len(ml_pair[1]), np.float32), ml_pair[1], ml_pair[0]),
                         shape=(671, 9125))
    m_ui = SparseRowArray.from_scipy(rmat, values=False)
    t2 = _accel.slim.train_slim(m_ui, m_ui.transpose(), 1.0, 1.0, 100, None)
    t2.cancel()
    with pytest.raises(RuntimeError, match="accelerator task failed"):
        run_accel_task(t2)


@pytest.fixture(scope="module")
def trained(gpu):
    from lkpy_amd.data import load_movielens_npz
    from lkpy_amd.knn import SLIMScorer

    ds = load_movielens_npz(GOLDEN / "ml_small.npz")
    scorer = SLIMScorer(max_nbrs=500)
    scorer.train(ds)
    return ds, scorer


def test_component(gpu, trained, ml_pair, ml_columns, ml_restated):
    from lkpy_amd.data import ItemList, RecQuery

    ds, scorer = trained
    w = scorer.weights
    assert isinstance(w, sps.csr_array) and w.shape == (9125, 9125)
    assert scorer.is_trained() and np.all(w.diagonal() == 0)
    # the transpose's rows are the restatement's on the sampled columns (the dataset's item
    # numbering is the fixture's: sorted item ids)
    wt = sps.csr_array(w.T.tocsr())
    wt.sort_indices()
    want = ml_restated[CONFIGS[1]][0]
    for r, c in enumerate(ml_columns):
        a, b = slice(wt.indptr[c], wt.indptr[c + 1]), slice(want[0][r], want[0][r + 1])
        assert np.array_equal(wt.indices[a], want[1][b])
        assert np.array_equal(wt.data[a].view(np.uint32), want[2][b].view(np.uint32))

    ids = ds.items.ids()
    n_items = len(ids)
    rng = np.random.default_rng(1)
    all_items = ItemList(item_ids=np.concatenate([ids, [10 ** 9]]))  # one unknown target

    def scipy_scores(nums):
        nums = nums[nums >= 0]
        x = sps.csr_array((np.ones(len(nums), np.float32), nums, [0, len(nums)]),
                          shape=(1, n_items))
        return (x @ w).toarray()[0, :]

    queries, wants = [], []
    for u in list(ds.users.ids()[:12]):
        hist = ds.user_row(u)
        queries.append(RecQuery(user_id=u, user_items=hist))
        wants.append(scipy_scores(hist.numbers(vocabulary=ds.items)))
    # unsorted, one item repeated, one unknown item
    h = rng.permutation(ds.user_row(ds.users.ids()[3]).ids())[:30]
    odd = np.concatenate([h, h[:1], [10 ** 9 + 1]])
    queries.append(RecQuery(user_items=ItemList(item_ids=odd)))
    wants.append(scipy_scores(ds.items.numbers(odd, missing="negative")))
    zeros = 0
    for q, want in zip(queries, wants):
        got = np.asarray(scorer(q, all_items).scores(), np.float32)
        assert np.array_equal(got[:n_items].view(np.uint32), want.view(np.uint32))
        assert np.isnan(got[n_items])  # unknown target
        zeros += int((got[:n_items] == 0.0).sum())
    assert zeros > 0  # known items no history item points at score 0.0, not NaN
    assert not np.isnan(wants[-1]).any()
    # a repeated history item counts twice (unlike EASE)
    once = scipy_scores(ds.items.numbers(np.concatenate([h, [10 ** 9 + 1]]), missing="negative"))
    assert not np.array_equal(once, wants[-1])

    # no history / an empty history: all NaN
    for q in (RecQuery(user_id=-5), RecQuery(user_items=ItemList(item_ids=ids[:0]))):
        assert np.isnan(np.asarray(scorer(q, all_items).scores())).all()

    # score_batch = the per-query calls; pickle round trip scores identically
    lists = [all_items] * len(queries)
    clone = pickle.loads(pickle.dumps(scorer))
    assert "_dev" not in clone.__dict__
    for s in (scorer, clone):
        for q, il, want in zip(queries, s.score_batch(queries, lists), wants):
            got = np.asarray(il.scores(), np.float32)
            assert np.array_equal(got[:n_items].view(np.uint32), want.view(np.uint32))


def test_recommend_through_slim_toml(gpu):
    from lkpy_amd import batch
    from lkpy_amd.data import load_movielens_npz
    from lkpy_amd.knn import SLIMScorer
    from lkpy_amd.pipeline import Pipeline

    ds = load_movielens_npz(GOLDEN / "ml_small.npz")
    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "slim.toml")
    pipe.train(ds)
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, SLIMScorer) and scorer.config.max_nbrs == 500
    w = scorer.weights
    n_items = w.shape[0]
    users = list(ds.users.ids()[:60]) + [int(ds.users.ids()[-1]), -7]  # the last one unknown
    n = 100
    calls = []
    orig = pipe.run
    pipe.run = lambda *a, **k: (calls.append(a), orig(*a, **k))[1]
    got = batch.recommend(pipe, users, n)
    pipe.run = orig
    assert not calls, "batch.recommend must not fall back to one pipeline run per user"
    assert len(got) == len(users)

    ties = zero_listed = 0
    for u in users:
        g = got.lookup(u)
        want = pipe.run("recommender", query=u, n=n)
        if u == -7:  # no history: nothing to recommend, either way
            assert len(g) == 0 and len(want) == 0
            continue
        gi = np.asarray(g.numbers(vocabulary=scorer.items))
        gs = np.asarray(g.scores(), np.float32)
        ws = np.asarray(want.scores(), np.float32)
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), u  # sorted score rows
        hist = ds.user_row(u).numbers(vocabulary=ds.items)
        # a host top-n of the SciPy scores with the history struck out
        x = sps.csr_array((np.ones(len(hist), np.float32), hist, [0, len(hist)]),
                          shape=(1, n_items))
        row = (x @ w).toarray()[0, :]
        cand = row.copy()
        cand[hist] = -np.inf
        top = np.sort(cand)[::-1][:n]
        assert len(gi) == n
        assert np.array_equal(gs.view(np.uint32), top.astype(np.float32).view(np.uint32))
        assert np.array_equal(row[gi].view(np.uint32), gs.view(np.uint32))  # item carries its score
        assert not np.isin(gi, hist).any() and len(np.unique(gi)) == len(gi)
        zero_listed += int((gs == 0.0).sum())
        if not np.array_equal(gi, np.asarray(want.numbers(vocabulary=scorer.items))):
            ties += 1
    print(f"\n{len(users)} users: lists differing among equal scores: {ties}; "
          f"listed items scoring exactly 0.0: {zero_listed}")

    # the HistoryBatch path and the list-of-queries path give the same arrays; small panels too
    from lkpy_amd.data import RecQuery

    lookup = pipe.node("history-lookup").component
    gi, gs = scorer.recommend_batch(lookup.batch(users), n)
    li, ls = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in users], n)
    assert np.array_equal(gi, li)
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint32),
                          np.ascontiguousarray(ls).view(np.uint32))
    assert (gi[-1] == -1).all() and np.isnan(gs[-1]).all()
    old = SLIMScorer.PANEL_BYTES
    try:
        SLIMScorer.PANEL_BYTES = 4 * n_items * 7  # panels of 7 queries
        pi, ps = scorer.recommend_batch(lookup.batch(users), n)
    finally:
        SLIMScorer.PANEL_BYTES = old
    assert np.array_equal(pi, gi)
    assert np.array_equal(np.ascontiguousarray(ps).view(np.uint32),
                          np.ascontiguousarray(gs).view(np.uint32))


def test_score_batch_small_panels_equal_one_panel(gpu, monkeypatch, trained):
    """``score_batch`` through panels of 7 queries -- 8 of 7 and one of 6, the query without
    history in the last -- gives one panel's scores bit for bit.  The 62 queries of
    ``test_recommend_through_slim_toml``; 40 targets each, one of them unknown."""
    from lkpy_amd import _device as D
    from lkpy_amd.basic import UserTrainingHistoryLookup
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.knn import SLIMScorer

    ds, scorer = trained
    lookup = UserTrainingHistoryLookup()
    lookup.train(ds)
    users = list(ds.users.ids()[:60]) + [int(ds.users.ids()[-1]), -7]  # the last one unknown
    queries = [lookup(RecQuery.create(u)) for u in users]
    ids = ds.items.ids()
    n_items = len(ids)
    rng = np.random.default_rng(11)
    lists, unknown_at = [], []
    for _ in users:
        unknown_at.append(int(rng.integers(0, 40)))
        lists.append(ItemList(item_ids=np.insert(rng.choice(ids, 39, replace=False),
                                                 unknown_at[-1], 10 ** 9)))
    assert len(queries) == 62 and scorer._panel_rows() >= 62
    one = scorer.score_batch(queries, lists)
    launched, score = [], D.slim_score_batch
    with monkeypatch.context() as m:
        m.setattr(D, "slim_score_batch",
                  lambda *a, **k: (launched.append(k.get("rows")), score(*a, **k))[1])
        m.setattr(SLIMScorer, "PANEL_BYTES", 4 * n_items * 7)  # panels of 7 queries
        small = scorer.score_batch(queries, lists)
    assert launched == [(lo, min(62, lo + 7)) for lo in range(0, 62, 7)] and len(launched) == 9
    assert [hi - lo for lo, hi in launched] == [7] * 8 + [6] and launched[-1] == (56, 62)
    assert len(one) == len(small) == 62
    finite = 0
    for a, b, il, at in zip(one, small, lists, unknown_at):
        assert np.array_equal(a.ids(), il.ids()) and np.array_equal(b.ids(), il.ids())
        sa = np.ascontiguousarray(a.scores(), dtype=np.float32)
        sb = np.ascontiguousarray(b.scores(), dtype=np.float32)
        assert sa.shape == (40,) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert np.isnan(sb[at])  # the unknown target
        finite += int(np.isfinite(sb).sum())
    assert np.isnan(np.asarray(small[-1].scores())).all()  # no history: every score NaN
    assert finite == 61 * 39  # every known target of a query with history has a score
