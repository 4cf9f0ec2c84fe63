"""
FlexMF explicit on the device (csrc/flexmf.hip, csrc/mf_pairs.hip, lkpy_amd/flexmf.py) against the
Torch / NumPy restatement of ``tests/flexmf_explicit_restatement.py``.

Bar of the step parity: the criterion of ``tests/test_gpu_flexmf.py`` -- the largest absolute
difference over all tables between the device and the FLOAT64 Torch restatement is at most 4 x
the distance of the FLOAT32 Torch restatement from the float64 one, computed in the same test from
the same inputs; the same for the per-step losses.  ``tests/test_flexmf_explicit_host.py`` shows
that the implicit step's item weight, or a loss reported with the norm term, lands four to five
orders of magnitude outside it.

Bar of a score: ``|got - want| <= 1e-5 max(|want|, sum |terms|)`` against the float64 inner
product, the bound ``test_gpu_flexmf.py::test_largest_embedding_size`` applies.
"""
import json
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

import flexmf_explicit_restatement as X

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
EXTRA_USERS = [900001, 900002]  # known to the vocabulary, no interactions


@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def centred(ml):
    from lkpy_amd.flexmf import centred_ratings

    return centred_ratings(ml)[1]


def _init(ds, k, seed=1):
    from lkpy_amd.flexmf import initial_tables

    gen = torch.Generator().manual_seed(seed)
    return initial_tables(ds.user_count, ds.item_count, k, gen, user_bias=True, item_bias=True,
                          user_counts=np.diff(ds._indptr),
                          item_counts=np.bincount(ds._cols, minlength=ds.item_count))


def _batches(ds, centred, epochs=2, B=8192, seed=3):
    "the fixed permutation handed to both sides"
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(epochs):
        perm = rng.permutation(len(ds._rows))
        for s in range(0, len(perm), B):
            sel = perm[s:s + B]
            out.append((ds._rows[sel], ds._cols[sel], centred[sel]))
    return out


def _run_device(tabs, batches, gpu, **kw):
    from lkpy_amd import _device as D

    st = D.FlexMFState(tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["u_bias.weight"],
                       tabs["i_bias.weight"], loss="mse", dev=gpu, **kw)
    losses = [st.step_explicit(u, i, r) for u, i, r in batches]
    return st.host_tables(), torch.cat(losses).cpu().numpy().astype(np.float64)


def _run_torch(tabs, batches, dtype, **kw):
    tr = X.TorchExplicitTrainer(tabs, dtype=dtype, **kw)
    losses = [tr.step(u, i, r) for u, i, r in batches]
    return tr.tables(), np.asarray(losses, np.float64)


def _parity(tabs, batches, gpu, what, **kw):
    f64, l64 = _run_torch(tabs, batches, torch.float64, **kw)
    f32, l32 = _run_torch(tabs, batches, torch.float32, **kw)
    dev, ldev = _run_device(tabs, batches, gpu, **kw)
    d32, ddev = X.table_distance(f32, f64), X.table_distance(dev, f64)
    e32, edev = float(np.abs(l32 - l64).max()), float(np.abs(ldev - l64).max())
    print(f"{what}: tables float32 {d32:.3e} device {ddev:.3e} (bound {4 * d32:.3e}); "
          f"losses float32 {e32:.3e} device {edev:.3e} (bound {4 * e32:.3e})")
    assert d32 > 0 and e32 > 0
    assert ddev <= 4.0 * d32, (what, ddev, d32)
    assert edev <= 4.0 * e32, (what, edev, e32)
    return dev, f64


def _hyper(reg_method):
    return dict(reg_method=reg_method, regularization=0.1, learning_rate=0.01)


# ---- the training step ------------------------------------------------------------------------
@pytest.mark.parametrize("reg_method,k", [("L2", 64), ("AdamW", 64), (None, 64), ("L2", 50),
                                          ("L2", 256)])
def test_step_parity(ml, centred, gpu, reg_method, k):
    "26 steps (two epochs of ml-latest-small at B = 8192) from the seeded initialisation"
    batches = _batches(ml, centred)
    short = len(ml._rows) % 8192  # each epoch ends in a short batch
    assert len(batches) == 26 and 0 < short == len(batches[12][0]) == len(batches[25][0])
    _parity(_init(ml, k), batches, gpu, f"{reg_method}/k={k}", **_hyper(reg_method))


@pytest.mark.parametrize("reg_method", ["L2", "AdamW"])
def test_one_user_batch(ml, gpu, reg_method):
    "a batch that is one user 8192 times, 200 of its samples one (user, item) pair"
    rng = np.random.default_rng(9)
    u = int(np.argmax(np.diff(ml._indptr)))
    batches = []
    for _ in range(3):
        items = rng.integers(0, ml.item_count, 8192).astype(np.int32)
        items[rng.permutation(8192)[:200]] = 77
        ratings = rng.normal(0.0, 1.0, 8192).astype(np.float32)
        batches.append((np.full(8192, u, np.int32), items, ratings))
    _parity(_init(ml, 64), batches, gpu, f"one user/{reg_method}", **_hyper(reg_method))


def test_batch_of_one_sample(ml, gpu):
    batches = [(ml._rows[i:i + 1], ml._cols[i:i + 1], np.array([r], np.float32))
               for i, r in ((5, 1.5), (5, -0.5), (40000, 0.25))]
    _parity(_init(ml, 64), batches, gpu, "one sample", **_hyper("L2"))


def test_zero_rows_under_l2(ml, centred, gpu):
    "a user row and an item row of norm exactly 0: the norm's gradient there is 0, not NaN"
    tabs = _init(ml, 64)
    rng = np.random.default_rng(4)
    sel = rng.permutation(len(ml._rows))[:4096]
    users, items = ml._rows[sel].copy(), ml._cols[sel].copy()
    zu, zi = int(users[0]), int(items[1])
    tabs["u_embed.weight"][zu] = 0.0
    tabs["i_embed.weight"][zi] = 0.0
    assert (users == zu).sum() >= 1 and (items == zi).sum() >= 1
    dev, f64 = _parity(tabs, [(users, items, centred[sel])] * 3, gpu, "zero rows", **_hyper("L2"))
    for name in X.TABLES:
        assert np.isfinite(dev[name]).all(), name
    # the rows moved (the data term alone moves them), and as Torch's did (_parity's bound)
    assert dev["u_embed.weight"][zu].any() and dev["i_embed.weight"][zi].any()
    assert f64["u_embed.weight"][zu].any() and f64["i_embed.weight"][zi].any()


def test_steps_are_reproducible(ml, centred, gpu):
    batches = _batches(ml, centred, epochs=1)
    for reg_method in ("L2", "AdamW"):
        a, la = _run_device(_init(ml, 64), batches, gpu, **_hyper(reg_method))
        b, lb = _run_device(_init(ml, 64), batches, gpu, **_hyper(reg_method))
        for name in a:
            assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
        assert np.array_equal(la, lb)


def test_state_rejects_the_other_step(ml, gpu):
    from lkpy_amd import _device as D

    tabs = _init(ml, 16)
    args = (tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["u_bias.weight"],
            tabs["i_bias.weight"])
    with pytest.raises(ValueError, match="step_explicit"):
        D.FlexMFState(*args, loss="mse", dev=gpu).step([0], [0], [[1]])
    with pytest.raises(ValueError, match="mse"):
        D.FlexMFState(*args, loss="logistic", dev=gpu).step_explicit([0], [0], [1.0])
    with pytest.raises(ValueError, match="outside"):
        D.FlexMFState(*args, loss="mse", dev=gpu).step_explicit([0], [ml.item_count], [1.0])


# ---- the trainer --------------------------------------------------------------------------------
def test_trainer_parameters_and_epoch_loss(ml, gpu):
    from lkpy_amd.flexmf import FlexMFExplicitConfig, FlexMFExplicitScorer, centred_ratings
    from lkpy_amd.training import TrainingOptions

    sc = FlexMFExplicitScorer(epochs=1)
    tr = sc.create_trainer(ml, TrainingOptions(rng=2))
    assert sc.global_bias == centred_ratings(ml)[0]
    # the reference's initial parameters bit for bit from the same seed
    want = _init(ml, 64, seed=2)
    p0 = tr.get_parameters()
    assert set(p0) == set(X.TABLES)
    for name in X.TABLES:
        assert np.array_equal(p0[name], want[name]), name
    first = tr.train_epoch()["loss"]
    # the restatement's first epoch from the same seed: the same permutation, no sampling.  The
    # epoch loss is a mean of batch losses, so it is held to the step parity's loss bound: 4 x the
    # largest float32-to-float64 distance of a batch loss of that epoch.
    l32, l64 = [], []
    X.train_explicit_restatement(ml, FlexMFExplicitConfig(epochs=1), 2, torch.float32, l32)
    X.train_explicit_restatement(ml, FlexMFExplicitConfig(epochs=1), 2, torch.float64, l64)
    e32 = float(np.abs(np.asarray(l32[0]) - np.asarray(l64[0])).max())
    want_first = float(np.mean(l32[0]))
    print(f"first epoch loss: device {first:.9f}, float32 restatement {want_first:.9f}, "
          f"float64 {np.mean(l64[0]):.9f}; bound {4 * e32:.3e}")
    assert e32 > 0 and abs(first - want_first) <= 4.0 * e32
    p1 = tr.get_parameters()
    second = tr.train_epoch()["loss"]
    assert 0.0 < second < first  # the squared error falls
    p2 = tr.get_parameters()
    tr.load_parameters(p0)
    assert np.array_equal(sc.item_embeddings, want["i_embed.weight"])
    assert np.array_equal(sc.user_bias, want["u_bias.weight"].reshape(-1))
    tr.load_parameters(p2)
    for name in X.TABLES:
        assert np.array_equal(tr.get_parameters()[name], p2[name]), name
        assert not np.array_equal(p1[name], p2[name]), name
    tr.finalize()
    assert np.array_equal(sc.user_embeddings, p2["u_embed.weight"])


# ---- the pair scorer ----------------------------------------------------------------------------
N_USERS, N_ITEMS = 300, 2000


def _random_scorer(k, seed=0):
    from lkpy_amd.data import Vocabulary
    from lkpy_amd.flexmf import FlexMFExplicitScorer

    rng = np.random.default_rng(seed)
    sc = FlexMFExplicitScorer(embedding_size=k)
    sc.users = Vocabulary(np.arange(1000, 1000 + N_USERS), "user")
    sc.items = Vocabulary(np.arange(50000, 50000 + N_ITEMS), "item")
    sc.user_embeddings = rng.normal(0, 0.5, (N_USERS, k)).astype(np.float32)
    sc.item_embeddings = rng.normal(0, 0.5, (N_ITEMS, k)).astype(np.float32)
    sc.user_bias = rng.normal(0, 0.3, N_USERS).astype(np.float32)
    sc.item_bias = rng.normal(0, 0.3, N_ITEMS).astype(np.float32)
    sc.global_bias = float(np.float32(3.5015717))
    return sc


def _want(sc, u, nums):
    "(float64 score, the size of what is summed) of user number u against item numbers"
    P, Q = sc.user_embeddings.astype(np.float64), sc.item_embeddings.astype(np.float64)
    want = sc.global_bias + sc.user_bias[u] + sc.item_bias[nums] + Q[nums] @ P[u]
    size = abs(sc.global_bias) + abs(sc.user_bias[u]) + np.abs(sc.item_bias[nums]) + \
        np.abs(Q[nums]) @ np.abs(P[u])
    return want, size


def _queries(seed=1):
    "37 queries: lists of 0, 1, 3, 63, 64, 65 and 1000 items and a mix; unknown users and items"
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(seed)
    lengths = [0, 1, 3, 63, 64, 65, 1000] + rng.integers(0, 120, 30).tolist()
    users = (1000 + rng.integers(0, N_USERS, len(lengths))).tolist()
    users[9], users[20] = -4, 999  # unknown users
    users[11] = None
    lists = []
    for q, n in enumerate(lengths):
        ids = 50000 + rng.choice(N_ITEMS, n, replace=False)
        if n >= 3 and q % 3 == 0:
            ids[rng.integers(0, n)] = 7  # an unknown item
            ids[0] = -9
        lists.append(ItemList(item_ids=ids))
    return users, lists


@pytest.mark.parametrize("k", [1, 50, 64, 256])
def test_pair_scores(gpu, k):
    sc = _random_scorer(k)
    users, lists = _queries()
    assert len(users) == 37
    got = sc.score_batch(users, lists)
    worst = 0.0
    for q, (uid, il, res) in enumerate(zip(users, lists, got)):
        s = res.scores()
        assert s.dtype == np.float32 and s.shape == (len(il),)
        assert np.array_equal(res.ids(), il.ids())
        u = None if uid is None else sc.users.number(uid, missing=None)
        nums = il.numbers(vocabulary=sc.items, missing="negative")
        known = nums >= 0 if u is not None else np.zeros(len(il), bool)
        assert np.array_equal(np.isnan(s), ~known), q  # NaN exactly at the unknown
        if known.any():
            want, size = _want(sc, u, nums[known])
            err = np.abs(s[known] - want) / np.maximum(np.abs(want), size)
            worst = max(worst, float(err.max()))
        # alone it has the bits it has in the batch
        alone = sc(uid, il).scores()
        assert alone.shape == s.shape
        assert np.array_equal(alone.view(np.uint32), s.view(np.uint32)), q
    print(f"k={k}: worst relative error {worst:.3e} (bound 1e-5)")
    assert worst <= 1e-5
    assert len(got[0]) == 0 and got[0].scores().shape == (0,)  # an empty list
    assert sc.score_batch([], []) == []
    assert sc.score_pairs([3], [0, 0], []).shape == (0,)


def test_pair_scores_by_number_many_short_lists(gpu):
    "5000 queries of 0..7 targets: more queries than one step of the offset search covers"
    sc = _random_scorer(64, seed=2)
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 8, 5000)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    unums = rng.integers(-1, N_USERS, 5000).astype(np.int32)
    inums = rng.integers(-1, N_ITEMS, int(ptr[-1])).astype(np.int32)
    got = sc.score_pairs(unums, ptr, inums)
    dev = sc.score_pairs(unums, ptr, inums, device_output=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), got.view(np.uint32))
    urep = np.repeat(unums, lengths)
    known = (urep >= 0) & (inums >= 0)
    assert np.array_equal(np.isnan(got), ~known)
    P, Q = sc.user_embeddings.astype(np.float64), sc.item_embeddings.astype(np.float64)
    u, i = urep[known], inums[known]
    dots, sizes = np.einsum("nk,nk->n", P[u], Q[i]), np.einsum("nk,nk->n", np.abs(P[u]), np.abs(Q[i]))
    want = sc.global_bias + sc.user_bias[u] + sc.item_bias[i] + dots
    size = abs(sc.global_bias) + np.abs(sc.user_bias[u]) + np.abs(sc.item_bias[i]) + sizes
    assert (np.abs(got[known] - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    for q in (0, 1, 63, 64, 65, 2500, 4999):  # a query alone: the same bits
        one = sc.score_pairs(unums[q:q + 1], [0, lengths[q]], inums[ptr[q]:ptr[q + 1]])
        assert np.array_equal(one.view(np.uint32), got[ptr[q]:ptr[q + 1]].view(np.uint32)), q
    with pytest.raises(ValueError, match="tgt_ptr"):
        sc.score_pairs(unums[:2], [0, 3, 2], inums[:2])


# ---- component ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split(ml):
    "200 users with a fifth of their rows held out; the training set knows two users more"
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.splitting import SampleFrac, sample_users

    sp = sample_users(ml, 200, SampleFrac(0.2, rng=5), rng=5)
    tr = sp.train
    users = Vocabulary(np.concatenate([tr.users.ids(), EXTRA_USERS]), "user")
    train = Dataset(users, tr.items, users.numbers(tr.users.ids(tr._rows)), tr._cols, tr._attrs)
    return train, sp.test


@pytest.fixture(scope="module")
def trained(split, gpu):
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "flexmf-explicit.toml")
    pipe.train(split[0], TrainingOptions(rng=13))
    return pipe


UNKNOWN_USER = -777


def _pairs(split):
    """the held-out lists of the 200 users, an unknown item in every fourth, the two users
    without interactions and a user the vocabulary does not know"""
    from lkpy_amd.data import ItemList

    train, test = split
    pairs = {}
    for n, (key, truth) in enumerate(test):
        ids = truth.ids()
        pairs[key.user_id] = ItemList(item_ids=np.concatenate([ids, [-5]]) if n % 4 == 0 else ids)
    for u in EXTRA_USERS + [UNKNOWN_USER]:
        pairs[u] = ItemList(item_ids=train.items.ids()[:7])
    return pairs


def test_component_predict(split, gpu, trained):
    """``batch.predict`` = the per-query ``rating-predictor``, bit for bit.  ``is_fallback`` marks
    what the scorer cannot score: unknown items and a user the vocabulary does not know.  A user
    the vocabulary knows but who has no interactions is scored by the model, as the reference's
    ``__call__`` does (_base.py:128-133 asks the vocabulary only): its row and bias are still
    zero, so its score is ``global_bias + b_i`` and no fallback."""
    from lkpy_amd import batch
    from lkpy_amd.flexmf import FlexMFExplicitScorer

    train, _ = split
    pipe = trained
    sc = pipe.node("scorer").component
    assert isinstance(sc, FlexMFExplicitScorer) and sc.is_trained() and sc.trained_epochs == 10
    P, Q = sc.user_embeddings, sc.item_embeddings
    assert P.shape == (train.user_count, 64) and Q.shape == (train.item_count, 64)
    assert P.dtype == np.float32 and np.isfinite(P).all() and np.isfinite(Q).all()
    assert sc.user_bias.shape == (train.user_count,) and sc.item_bias.shape == (train.item_count,)
    r = torch.from_numpy(np.ascontiguousarray(train._attrs["rating"], dtype=np.float32))
    assert isinstance(sc.global_bias, float) and sc.global_bias == r.mean().item()
    # users without interactions start at zero and are in no batch: SparseAdam leaves them there
    empty = train.users.numbers(np.asarray(EXTRA_USERS))
    assert not P[empty].any() and not sc.user_bias[empty].any()

    pairs = _pairs(split)
    assert len(pairs) == 203
    calls = []
    orig = sc.score_batch
    sc.score_batch = lambda q, il: (calls.append(len(q)), orig(q, il))[1]
    try:
        out = batch.predict(pipe, pairs)
    finally:
        del sc.score_batch
    assert calls == [203]  # one call for the whole batch
    n_fallback = 0
    for n, (u, il) in enumerate(pairs.items()):
        one = pipe.run("rating-predictor", query=u, items=il)
        got = out.lookup(u)
        assert np.array_equal(got.ids(), il.ids())
        assert np.array_equal(got.scores().view(np.uint32), one.scores().view(np.uint32)), u
        fb = got.field("is_fallback")
        assert np.array_equal(fb, one.field("is_fallback"))
        assert np.array_equal(fb, np.isin(il.ids(), [-5]) | (u == UNKNOWN_USER)), u
        assert np.isfinite(got.scores()).all()
        if u in EXTRA_USERS:
            want = np.float32(sc.global_bias) + sc.item_bias[:7]
            assert np.abs(got.scores() - want).max() <= 1e-6
        n_fallback += int(fb.sum())
    assert n_fallback == 50 + 7


def test_component_recommend_and_pickle(split, gpu, trained):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    train, test = split
    pipe = trained
    sc = pipe.node("scorer").component
    uids = np.asarray([key.user_id for key, _ in test][:40] + EXTRA_USERS[:1] + [UNKNOWN_USER])
    recs = batch.recommend(pipe, uids, 10)
    for u in uids[:40]:
        il = recs.lookup(u)
        assert len(il) == 10
        nums = il.numbers(vocabulary=train.items)
        un = train.users.number(u)
        assert not np.isin(nums, train._cols[train._indptr[un]:train._indptr[un + 1]]).any()
        got = il.scores()
        assert (np.diff(got) <= 0).all()
        want, size = _want(sc, un, nums)  # (global bias included)
        assert (np.abs(got - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
        again = sc(u, ItemList(item_ids=il.ids())).scores()
        assert (np.abs(got - again) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    none = recs.lookup(UNKNOWN_USER)
    assert none is None or len(none) == 0
    idx, val = sc.recommend_batch([int(uids[0]), UNKNOWN_USER], 5, exclude_history=False)
    assert idx.shape == (2, 5) and (idx[1] == -1).all() and np.isnan(val[1]).all()
    dev_idx, dev_val = sc.recommend_batch([int(uids[0])], 5, exclude_history=False,
                                          device_output=True)
    assert dev_idx.is_cuda and np.array_equal(dev_idx.cpu().numpy()[0], idx[0])

    # a pickle round trip holds no device state and scores the same bits
    items = ItemList(item_ids=np.concatenate([train.items.ids()[:300], [-5, -6]]))
    got = sc(uids[3], items).scores()
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__ and "_pending_sync" not in sc2.__dict__
    assert sc2.global_bias == sc.global_bias
    assert np.array_equal(sc2(uids[3], items).scores().view(np.uint32), got.view(np.uint32))
    assert np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()
    assert np.isnan(sc(-12345, items).scores()).all() and np.isnan(sc(None, items).scores()).all()


def test_retrain_false_skips(split, gpu, trained):
    from lkpy_amd.training import TrainingOptions

    sc = trained.node("scorer").component
    before = sc.item_embeddings
    sc.train(split[0], TrainingOptions(retrain=False, rng=99))
    assert sc.item_embeddings is before


# ---- quality --------------------------------------------------------------------------------
def test_quality(ml, gpu):
    """The pooled test RMSE of the device scorer from three fixed seeds against the float32 Torch
    restatement trainer's five CPU runs on the same split
    (tests/golden/flexmf_explicit_quality.json): each run at most their worst plus their range,
    and the mean below the ``BiasScorer`` alone (which the restatement's runs all beat)."""
    from lkpy_amd.flexmf import FlexMFExplicitScorer
    from lkpy_amd.splitting import SampleFrac, sample_users
    from lkpy_amd.training import TrainingOptions

    gold = json.loads((GOLDEN / "flexmf_explicit_quality.json").read_text())
    ref = np.asarray(gold["rmse"])
    assert ref.max() < gold["bias_rmse"]
    ceiling = ref.max() + (ref.max() - ref.min())
    seed = gold["split_seed"]  # (the maker's split)
    sp = sample_users(ml, ml.user_count // 5, SampleFrac(0.2, rng=seed), rng=seed)
    assert sp.test_size == gold["test_ratings"]
    keys = [key.user_id for key, _ in sp.test]
    lists = [truth for _, truth in sp.test]
    truth = np.concatenate([np.asarray(il.field("rating"), np.float64) for il in lists])
    vals = []
    for seed in (1, 2, 3):
        sc = FlexMFExplicitScorer()
        sc.train(sp.train, TrainingOptions(rng=seed))
        pred = np.concatenate([il.scores() for il in sc.score_batch(keys, lists)])
        assert np.isfinite(pred).all()
        vals.append(float(np.sqrt(np.mean((pred.astype(np.float64) - truth) ** 2))))
    print(f"RMSE {[round(v, 4) for v in vals]}, mean {np.mean(vals):.4f}; restatement "
          f"{[round(v, 4) for v in ref]}; ceiling {ceiling:.4f}, bias alone "
          f"{gold['bias_rmse']:.4f}")
    assert max(vals) <= ceiling
    assert np.mean(vals) < gold["bias_rmse"]
