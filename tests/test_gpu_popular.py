"""The Popular and Random baselines on the device: ``lk_shared_order_topn`` against the NumPy
restatement (``tests/popular_restatement.py``), item numbers and score bits exactly; ``PopScorer``,
``TimeBoundedPopScore`` and ``RandomSelector`` through ``batch.recommend`` against the per-user
pipeline."""

from __future__ import annotations

import sys
from datetime import datetime, timedelta
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import popular_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"

# the kernel can go wrong at its 64-entry chunks, its four-wave workgroups and the ends of `order`
ORDER_LENGTHS = [0, 1, 63, 64, 65, 200]
LIST_LENGTHS = [1, 63, 64, 65, 100, -1]
BATCHES = [1, 5, 9]
N_KINDS = 6
UNIFORM_SEED = 20240607  # chi2 of the NumPy restatement of the keys for this seed: 54.0 (< 111.1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scores(kind: str, L: int):
    "L scored items and three NaN-scored ones (item numbers 0, L // 2 + 1 and the last)"
    n_items = L + 3
    rng = np.random.default_rng(1000 + L)
    if kind == "ties":
        s = rng.integers(0, 3, n_items).astype(np.float32)
    else:  # arbitrary float32 bit patterns minus the NaNs, plus +-inf and the two zeros
        s = rng.integers(0, 2 ** 32, n_items, dtype=np.uint64).astype(np.uint32).view(np.float32)
        s = s.copy()
        bad = np.isnan(s)
        s[bad] = rng.standard_normal(int(bad.sum())).astype(np.float32)
        special = np.array([np.inf, -np.inf, -0.0, 0.0, -0.0, 0.0], np.float32)
        at = np.arange(2, n_items - 1, max(1, (n_items - 3) // len(special)))[:len(special)]
        s[at] = special[:len(at)]
    s[[0, L // 2 + 1, n_items - 1]] = np.nan
    assert int((~np.isnan(s)).sum()) == L
    return s


def _histories(order, n_items: int):
    """The six kinds of history as (rows of a matrix, the history the rule sees): empty | the
    first 130 entries of the order | every item | repeated item numbers | a row that is asked for
    as row number -1 | a NaN-scored item (number 0) among scored ones."""
    L = len(order)
    rep = np.sort(order[[0, 0, L // 2, L // 2, L // 2, L - 1]]) if L else np.zeros(0, np.int32)
    mat = [np.zeros(0, np.int32), np.sort(order[:130]), np.arange(n_items, dtype=np.int32), rep,
           np.sort(order[:7]), np.sort(np.concatenate([[0], order[1:4]])).astype(np.int32)]
    seen = [m if k != 4 else None for k, m in enumerate(mat)]
    return [np.asarray(m, np.int32) for m in mat], seen


def _csr(rows, dtype, dev, n_items):
    from lkpy_amd import _device as D

    ptr = np.zeros(len(rows) + 1, dtype)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return D.DeviceCSR.from_arrays(ptr, idx, None, (len(rows), n_items), dev)


@pytest.mark.parametrize("wide", [False, True], ids=["ptr32", "ptr64"])
@pytest.mark.parametrize("kind", ["ties", "bits"])
def test_kernel_against_restatement(gpu, kind, wide):
    import torch

    from lkpy_amd import _device as D

    dtype = np.int64 if wide else np.int32
    shift = 0
    for L in ORDER_LENGTHS:
        scores = _scores(kind, L)
        n_items = len(scores)
        order = R.order(scores)
        assert len(order) == L
        d_order = torch.from_numpy(order).to(gpu)
        d_osc = torch.from_numpy(scores[order]).to(gpu)
        mat, seen = _histories(order, n_items)
        d_mat = _csr(mat, dtype, gpu, n_items)
        assert d_mat.is64 == wide
        for B in BATCHES:
            for n in LIST_LENGTHS:
                kinds = [(b + shift) % N_KINDS for b in range(B)]
                shift += 1
                want_i, want_s = R.lists(order, scores, [seen[k] for k in kinds], n)
                # (a) rows of the matrix by number, kind 4 as row number -1
                rows = np.array([k if k != 4 else -1 for k in kinds], np.int32)
                idx, sc = D.shared_order_topn(d_order, d_osc, n, B, hist=d_mat,
                                              rows=torch.from_numpy(rows).to(gpu))
                where = f"{kind} L={L} B={B} n={n} kinds={kinds}"
                assert idx.shape == want_i.shape == (B, L if n < 0 else n), where
                assert np.array_equal(idx.cpu().numpy(), want_i), where
                assert np.array_equal(_bits(sc.cpu().numpy()), _bits(want_s)), where
                # (b) no row numbers: list b reads row b of a CSR of its own
                own = _csr([mat[k] if k != 4 else mat[0] for k in kinds], dtype, gpu, n_items)
                idx, sc = D.shared_order_topn(d_order, d_osc, n, B, hist=own)
                assert np.array_equal(idx.cpu().numpy(), want_i), where
                assert np.array_equal(_bits(sc.cpu().numpy()), _bits(want_s)), where
        # no history at all: every row is the plain top of the order
        idx, sc = D.shared_order_topn(d_order, d_osc, 65, 5)
        want_i, want_s = R.lists(order, scores, [None] * 5, 65)
        assert np.array_equal(idx.cpu().numpy(), want_i)
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(want_s))


@pytest.mark.parametrize("kind", ["ties", "bits"])
def test_device_order_is_the_restatements(gpu, kind):
    "the order a trained model keeps in HBM: score descending, -0.0 and +0.0 tie, lower number first"
    from lkpy_amd.basic import PopScorer
    from lkpy_amd.data import Vocabulary

    for L in (0, 65, 200):
        scorer = PopScorer()
        scorer.item_scores = _scores(kind, L)
        scorer.items = Vocabulary(np.arange(len(scorer.item_scores)), "item")
        st = scorer._device_order()
        order = R.order(scorer.item_scores)
        assert np.array_equal(st["order"].cpu().numpy(), order)
        assert np.array_equal(_bits(st["order_scores"].cpu().numpy()),
                              _bits(scorer.item_scores[order]))
        assert scorer._device_order() is st  # (kept until the model is trained again)


# ---- through the components -------------------------------------------------------------------
@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _users(ds):
    return [int(u) for u in ds.users.ids()[::12]] + [10 ** 7]  # (the last one is unknown)


def _same_lists(pipe, out, users, n):
    for u in users:
        one = pipe.run("recommender", query=u, n=n)
        got = out.lookup(u)
        assert np.array_equal(got.ids(), one.ids()), u
        assert np.array_equal(_bits(got.scores()), _bits(one.scores())), u


@pytest.mark.parametrize("mode", ["quantile", "rank", "count"])
def test_batch_recommend_is_the_pipeline_per_user(gpu, ml_ds, mode):
    from lkpy_amd import batch
    from lkpy_amd.basic import PopScorer
    from lkpy_amd.data import RecQuery
    from lkpy_amd.pipeline import topn_pipeline

    pipe = topn_pipeline(PopScorer(score=mode))
    pipe.train(ml_ds)
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    users = _users(ml_ds)
    out = batch.recommend(pipe, users, 100)
    assert len(out) == len(users) and all(len(il) == 100 for il in out.lists())
    _same_lists(pipe, out, users, 100)
    assert len(ml_ds.user_row(users[0])) > 0
    assert not np.isin(out.lookup(users[0]).ids(), ml_ds.user_row(users[0]).ids()).any()
    # n above the item count: short lists, every candidate ranked
    long = batch.recommend(pipe, users, 10_000)
    assert len(long.lookup(users[-1])) == ml_ds.item_count
    assert len(long.lookup(users[0])) == ml_ds.item_count - len(
        np.unique(ml_ds.user_row(users[0]).ids()))
    _same_lists(pipe, long, users[::7] + users[-1:], 10_000)
    # a plain list of queries (rows = NULL, histories packed on the host)
    idx, sc = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in users], 100)
    hb_idx, hb_sc = scorer.recommend_batch(lookup.batch(users), 100)
    assert idx.shape == (len(users), 100)
    assert np.array_equal(idx, hb_idx) and np.array_equal(_bits(sc), _bits(hb_sc))
    for b, u in enumerate(users):
        assert np.array_equal(ml_ds.items.ids(idx[b]), out.lookup(u).ids())
    # nothing excluded: every row is the same list, the unknown user's
    idx, sc = scorer.recommend_batch(lookup.batch(users), 100, exclude_history=False)
    assert (idx == idx[-1]).all() and (_bits(sc) == _bits(sc[-1])).all()
    assert np.array_equal(ml_ds.items.ids(idx[-1]), out.lookup(users[-1]).ids())
    on_dev = scorer.recommend_batch(lookup.batch(users), 100, device_output=True)
    assert on_dev[0].is_cuda and np.array_equal(on_dev[0].cpu().numpy(), hb_idx)


def _stamped_synthetic():
    from lkpy_amd.data import Dataset

    rng = np.random.default_rng(5)
    users = rng.integers(0, 40, 900)
    items = np.minimum(rng.geometric(0.05, 900), 69)
    stamps = 1_600_000_000 + rng.integers(0, 1_000_000, 900)
    return Dataset.from_arrays(users, items, all_item_ids=np.arange(0, 72), timestamp=stamps)


def test_time_bounded_batch_is_the_pipeline_per_user(gpu):
    from lkpy_amd import batch
    from lkpy_amd.basic import TimeBoundedPopScore
    from lkpy_amd.pipeline import topn_pipeline

    ds = _stamped_synthetic()
    assert ds.has_duplicates  # (repeated item numbers inside the training rows)
    users = [int(u) for u in ds.users.ids()[::3]] + [999]
    cutoff = datetime(1970, 1, 1) + timedelta(seconds=1_600_500_000)
    for mode in ("quantile", "count"):
        pipe = topn_pipeline(TimeBoundedPopScore(score=mode, cutoff=cutoff))
        pipe.train(ds)
        scores = pipe.node("scorer").component.item_scores
        late = ds._attrs["timestamp"] > 1_600_500_000
        assert np.array_equal(np.bincount(ds._cols[late], minlength=72) > 0,
                              scores > 0) and 0 < late.sum() < 900
        for n in (10, -1):
            _same_lists(pipe, batch.recommend(pipe, users, n), users, n)
    # no interaction after the cutoff: NaN scores, empty lists from both paths
    pipe = topn_pipeline(TimeBoundedPopScore(cutoff=datetime(2030, 1, 1)))
    pipe.train(ds)
    assert np.isnan(pipe.node("scorer").component.item_scores).all()
    out = batch.recommend(pipe, users, 10)
    assert len(out) == len(users)
    for u in users:
        assert len(out.lookup(u)) == 0 and len(pipe.run("recommender", query=u, n=10)) == 0


# ---- panels -----------------------------------------------------------------------------------
def test_panels_and_the_stochastic_ranker(gpu, ml_ds):
    from lkpy_amd import batch
    from lkpy_amd.basic import PopScorer
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    pipe = topn_pipeline(PopScorer())
    pipe.train(ml_ds)
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    users = _users(ml_ds)[::3] + [10 ** 7]
    panel, valid, hist = scorer.dense_scores_batch(lookup.batch(users))
    assert panel.is_contiguous() and panel.shape == (len(users), ml_ds.item_count)
    assert valid.all() and valid.shape == (len(users),)
    assert (_bits(panel.cpu().numpy()) == _bits(scorer.item_scores)[None]).all()
    lens = np.diff(hist.h_indptr)
    assert lens[-1] == 0 and lens[0] == len(ml_ds.user_row(users[0]))
    # popularity-proportional sampling: the batch paths against the pipeline per user
    pipe.replace_component("ranker", StochasticTopNRanker(rng=(7, "user")),
                           query="history-lookup")
    ranker = pipe.node("ranker").component
    out = batch.recommend(pipe, users, 20)
    many = batch.recommend_samples(pipe, users, 20, 2)
    assert len(many) == 2 * len(users)
    for u in users:
        one = pipe.run("recommender", query=u, n=20)
        assert len(one) == 20
        assert np.array_equal(out.lookup(u).ids(), one.ids())
        assert np.array_equal(_bits(out.lookup(u).scores()), _bits(one.scores()))
        got = pipe.run_all("history-lookup", "scorer", query=u)
        two = ranker.sample(got["scorer"], got["history-lookup"], 20, samples=2)
        for s in range(2):
            assert np.array_equal(many.lookup(u, s).ids(), two[s].ids())
            assert np.array_equal(_bits(many.lookup(u, s).scores()), _bits(two[s].scores()))
    assert any(not np.array_equal(many.lookup(u, 0).ids(), many.lookup(u, 1).ids())
               for u in users)


# ---- Random -----------------------------------------------------------------------------------
def test_random_pipeline_batch_is_the_pipeline_per_user(gpu, ml_ds):
    from lkpy_amd import batch
    from lkpy_amd.pipeline import random_pipeline

    pipe = random_pipeline(n=20, rng=(7, "user"))
    pipe.train(ml_ds)
    users = _users(ml_ds)
    out = batch.recommend(pipe, users, None)
    small = batch.recommend(pipe, users, None, batch_size=7)
    assert len(out) == len(users) and out.key_fields == ("user_id",)
    differ = 0
    for u in users:
        il = out.lookup(u)
        one = pipe.run("recommender", query=u)
        assert np.array_equal(il.ids(), one.ids()), u
        assert np.array_equal(small.lookup(u).ids(), il.ids())
        assert il.scores() is None and one.scores() is None
        assert len(il) == 20 and len(set(il.ids().tolist())) == 20
        row = ml_ds.user_row(u)
        if row is not None:
            assert not np.isin(il.ids(), row.ids()).any()
        differ += not np.array_equal(il.ids(), out.lookup(users[0]).ids())
    assert differ >= len(users) - 2
    # an explicit n overrides the configured one, in both paths
    five = batch.recommend(pipe, users[:4], 5)
    for u in users[:4]:
        assert np.array_equal(five.lookup(u).ids(), pipe.run("recommender", query=u, n=5).ids())
        assert np.array_equal(five.lookup(u).ids(), out.lookup(u).ids()[:5])


def test_random_permutes_every_candidate(gpu):
    from lkpy_amd import batch
    from lkpy_amd.data import Dataset, ItemList, RecQuery
    from lkpy_amd.basic import RandomSelector
    from lkpy_amd.pipeline import random_pipeline

    rng = np.random.default_rng(3)
    ds = Dataset.from_arrays(rng.integers(0, 12, 150), rng.integers(100, 140, 150),
                             all_item_ids=np.arange(100, 140))
    pipe = random_pipeline(rng=(7, "user"))
    pipe.train(ds)
    users = [int(u) for u in ds.users.ids()] + [77]
    out = batch.recommend(pipe, users, None)
    for u in users:
        row = ds.user_row(u)
        cand = np.setdiff1d(np.arange(100, 140), [] if row is None else row.ids())
        il = out.lookup(u)
        assert len(il) == len(cand) and np.array_equal(np.sort(il.ids()), cand)
        assert np.array_equal(il.ids(), pipe.run("recommender", query=u).ids())
    assert len(out.lookup(77)) == 40  # an unknown user: every item is a candidate
    # n above the candidates: min(n, candidates)
    assert len(batch.recommend(pipe, users, 1000).lookup(users[0])) == len(out.lookup(users[0]))
    # one list: the input's fields are kept, no score is added
    sel = RandomSelector(n=6, rng=(7, "user"))
    items = ItemList(item_ids=np.arange(100, 110), rating=np.arange(10, dtype=np.float32))
    got = sel(items, RecQuery.create(3))
    assert len(got) == 6 and got.scores() is None
    assert np.array_equal(got.field("rating"), (got.ids() - 100).astype(np.float32))
    assert np.array_equal(sel(items, 3).ids(), got.ids()) and len(sel(items, 3, n=-1)) == 10


def test_random_first_position_is_uniform(gpu):
    "20 000 counted streams over 50 candidates: chi2 of the first position against chi2_49"
    import torch
    from scipy.stats import chi2

    from lkpy_amd.basic import RandomSelector

    sel = RandomSelector(rng=UNIFORM_SEED)
    assert not sel.by_user
    panel = torch.ones((20_000, 50), dtype=torch.float32, device=gpu)
    idx, _ = sel.rank_panel(panel, sel.streams(None, 20_000), 1)
    counts = np.bincount(idx.reshape(-1), minlength=50)
    stat = float(((counts - 400.0) ** 2 / 400.0).sum())
    print(f"chi2 of the first-position counts = {stat:.2f}")
    assert counts.sum() == 20_000 and stat < chi2.ppf(1 - 1e-6, 49)
