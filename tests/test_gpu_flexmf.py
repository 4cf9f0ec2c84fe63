"""
FlexMF implicit on the device (csrc/flexmf.hip, lkpy_amd/flexmf.py) against the Torch / NumPy
restatement of ``tests/flexmf_restatement.py``.

Bar of the step parity: the largest absolute difference over all tables between the device and
the FLOAT64 Torch restatement is at most 4 x the distance of the FLOAT32 Torch restatement from
the float64 one, computed in the same test from the same inputs.  Why 4: measured on the CPU the
float32 distance is 2.1e-6 .. 7.1e-6 for AdamW and 2.9e-7 .. 5.0e-7 for the sparse paths on
parameters of size 0.5, and a float32 run with every batch reordered lands 0.5 .. 1.1 times that
far from the original float32 run -- so 4 leaves room for another summation order, while a wrong
formula moves parameters by the order of lr = 1e-2 (tests/test_flexmf_host.py shows > 100 x).
"""
import json
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

import flexmf_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
PRESET_TOMLS = ["flexmf-bpr", "flexmf-logistic", "flexmf-warp"]


@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _init(ds, k, user_bias, item_bias, seed=1):
    from lkpy_amd.flexmf import initial_tables

    gen = torch.Generator().manual_seed(seed)
    return initial_tables(ds.user_count, ds.item_count, k, gen, user_bias=user_bias,
                          item_bias=item_bias, user_counts=np.diff(ds._indptr),
                          item_counts=np.bincount(ds._cols, minlength=ds.item_count))


def _batches(ds, n_neg, epochs=2, B=8192, seed=3, warp=False):
    "the fixed permutation, negatives (and WARP weights) handed to both sides"
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(epochs):
        perm = rng.permutation(len(ds._rows))
        for s in range(0, len(perm), B):
            sel = perm[s:s + B]
            neg = rng.integers(0, ds.item_count, (len(sel), n_neg)).astype(np.int32)
            w = R.warp_weights(rng.integers(1, 201, len(sel)), ds.item_count) if warp else None
            out.append((ds._rows[sel], ds._cols[sel], neg, w))
    return out


def _device_state(tabs, gpu, **kw):
    from lkpy_amd import _device as D

    return D.FlexMFState(tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["u_bias.weight"],
                         tabs["i_bias.weight"], dev=gpu, **kw)


def _run_device(tabs, batches, gpu, **kw):
    st = _device_state(tabs, gpu, **kw)
    losses = [st.step(u, p, n, w) for u, p, n, w in batches]
    return st.host_tables(), torch.cat(losses).cpu().numpy().astype(np.float64)


def _run_torch(tabs, batches, dtype, **kw):
    kw = dict(kw)
    kw.pop("negative_count", None)
    tr = R.TorchTrainer(tabs, dtype=dtype, **kw)
    losses = [tr.step(u, p, n, w) for u, p, n, w in batches]
    return tr.tables(), np.asarray(losses, np.float64)


def _parity(tabs, batches, gpu, what, **kw):
    f64, l64 = _run_torch(tabs, batches, torch.float64, **kw)
    f32, l32 = _run_torch(tabs, batches, torch.float32, **kw)
    dev, ldev = _run_device(tabs, batches, gpu, **kw)
    d32, ddev = R.table_distance(f32, f64), R.table_distance(dev, f64)
    e32, edev = float(np.abs(l32 - l64).max()), float(np.abs(ldev - l64).max())
    print(f"{what}: tables float32 {d32:.3e} device {ddev:.3e} (bound {4 * d32:.3e}); "
          f"losses float32 {e32:.3e} device {edev:.3e} (bound {4 * e32:.3e})")
    assert d32 > 0 and e32 > 0
    assert ddev <= 4.0 * d32, (what, ddev, d32)
    assert edev <= 4.0 * e32, (what, edev, e32)
    return dev


STEP_CONFIGS = [(rm, loss, 1, 64) for rm in ("AdamW", "L2", None)
                for loss in ("pairwise", "logistic")] + \
    [("AdamW", "warp", 1, 64), ("L2", "logistic", 3, 64), ("AdamW", "pairwise", 1, 50)]


@pytest.mark.parametrize("reg_method,loss,n_neg,k", STEP_CONFIGS)
def test_step_parity(ml, gpu, reg_method, loss, n_neg, k):
    "26 steps (two epochs of ml-latest-small at B = 8192) from the seeded initialisation"
    tabs = _init(ml, k, user_bias=loss == "logistic", item_bias=True)
    batches = _batches(ml, n_neg, warp=loss == "warp")
    assert len(batches) == 26
    _parity(tabs, batches, gpu, f"{reg_method}/{loss}/n={n_neg}/k={k}", loss=loss,
            reg_method=reg_method, regularization=0.01, learning_rate=0.01,
            negative_count=n_neg, positive_weight=1.0)


@pytest.mark.parametrize("reg_method,loss", [("AdamW", "logistic"), ("L2", "pairwise")])
def test_steps_are_reproducible(ml, gpu, reg_method, loss):
    tabs = _init(ml, 64, True, True)
    batches = _batches(ml, 1, epochs=1)
    kw = dict(loss=loss, reg_method=reg_method, negative_count=1)
    a, la = _run_device(tabs, batches, gpu, **kw)
    b, lb = _run_device(tabs, batches, gpu, **kw)
    for name in a:
        if a[name] is not None:
            assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
    assert np.array_equal(la, lb)


@pytest.mark.parametrize("reg_method", ["AdamW", "L2"])
def test_one_user_batch(ml, gpu, reg_method):
    "a batch that is one user 8192 times, with a negative equal to its positive"
    tabs = _init(ml, 64, True, True)
    rng = np.random.default_rng(9)
    u = int(np.argmax(np.diff(ml._indptr)))
    batches = []
    for _ in range(3):
        pos = rng.integers(0, ml.item_count, 8192).astype(np.int32)
        neg = rng.integers(0, ml.item_count, (8192, 1)).astype(np.int32)
        neg[:100, 0] = pos[:100]
        neg[100:200, 0] = pos[300:400]  # ... and equal to another sample's item
        batches.append((np.full(8192, u, np.int32), pos, neg, None))
    _parity(tabs, batches, gpu, f"one user/{reg_method}", loss="logistic", reg_method=reg_method,
            regularization=0.01, learning_rate=0.01, negative_count=1, positive_weight=2.0)


def _bits_for(n):
    b = 1
    while b < 32 and (1 << b) < n:
        b += 1
    return b


@pytest.mark.parametrize("reg_method", ["AdamW", "L2"])
def test_step_parity_at_other_sort_sizes(gpu, reg_method):
    """Synthetic tables whose per-batch sorts are not the 2 + 2 passes of every other case here:
    200 users (8 key bits, one pass) and 70 000 items (17 bits, three passes), batches of 4097
    samples (two tiles of the sort, the second holding one key) with one negative each (8194 item
    keys: three tiles, the third holding two); one batch is a single user throughout, with
    negatives equal to their positives."""
    from lkpy_amd.flexmf import initial_tables

    n_users, n_items, k, B, tile = 200, 70_000, 8, 4097, 4096
    assert (_bits_for(n_users) + 7) // 8 == 1 and (_bits_for(n_items) + 7) // 8 == 3
    assert ((B + tile - 1) // tile, B % tile) == (2, 1)
    assert ((2 * B + tile - 1) // tile, (2 * B) % tile) == (3, 2)
    tabs = initial_tables(n_users, n_items, k, torch.Generator().manual_seed(7), user_bias=True,
                          item_bias=True)
    rng = np.random.default_rng(21)
    batches = []
    for b in range(3):
        users = rng.integers(0, n_users, B).astype(np.int32)
        pos = rng.integers(0, n_items, B).astype(np.int32)
        neg = rng.integers(0, n_items, (B, 1)).astype(np.int32)
        if b == 1:
            users[:] = 137
            neg[:100, 0] = pos[:100]
            neg[100:200, 0] = pos[300:400]  # ... and equal to another sample's item
        batches.append((users, pos, neg, None))
    assert len(batches) == 3 and all(len(u) == B and n.shape == (B, 1) for u, _p, n, _w in batches)
    assert len(np.unique(batches[1][0])) == 1 and len(np.unique(batches[0][0])) == n_users
    assert (batches[1][2][:100, 0] == batches[1][1][:100]).all()
    assert max(int(p.max()) for _u, p, _n, _w in batches) >= 1 << 16  # the third digit is in use
    _parity(tabs, batches, gpu, f"sort sizes/{reg_method}", loss="logistic",
            reg_method=reg_method, regularization=0.01, learning_rate=0.01, negative_count=1,
            positive_weight=2.0)


# ---- sampler ------------------------------------------------------------------------------
def _dev_csr(indptr, cols, gpu):
    return (torch.from_numpy(np.asarray(indptr, np.int64)).to(gpu),
            torch.from_numpy(np.asarray(cols, np.int32)).to(gpu))


def test_sampler_never_returns_a_training_item_on_a_sparse_matrix(gpu):
    from lkpy_amd import _device as D

    rng = np.random.default_rng(0)
    n_users, n_items = 500, 2000
    lens = rng.integers(0, 100, n_users)  # at most 5 % of the items: c^11 < 5e-15 per draw
    indptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(n_items, m, replace=False)) for m in lens])
    keys = R.pair_keys(indptr, cols, n_items)
    rows = rng.integers(0, n_users, 100000).astype(np.int32)
    dp, dc = _dev_csr(indptr, cols, gpu)
    for weighting in ("uniform", "popular"):
        out = D.flexmf_sample_negatives(dp, dc, n_items, rows, 3, weighting, 123, 7).cpu().numpy()
        assert out.shape == (100000, 3) and out.dtype == np.int32
        assert out.min() >= 0 and out.max() < n_items
        assert not R.reject(keys, n_items, np.repeat(rows, 3), out.reshape(-1)).any()
    raw = D.flexmf_sample_negatives(dp, dc, n_items, rows, 3, "uniform", 123, 7,
                                    verify=False).cpu().numpy()
    assert R.reject(keys, n_items, np.repeat(rows, 3), raw.reshape(-1)).any()  # (what verify removes)


def test_sampler_false_negatives_on_ml_small(ml, gpu):
    "false negatives are at most 3 + 10 E, E = sum over the sampled rows of (row share)^11"
    from lkpy_amd import _device as D

    rows = ml._rows[np.random.default_rng(1).permutation(len(ml._rows))[:65536]]
    share = np.diff(ml._indptr)[rows] / ml.item_count
    E = float((share ** 11).sum())
    keys = R.pair_keys(ml._indptr, ml._cols, ml.item_count)
    dp, dc = _dev_csr(ml._indptr, ml._cols, gpu)
    out = D.flexmf_sample_negatives(dp, dc, ml.item_count, rows, 1, "uniform", 5, 0).cpu().numpy()
    false_neg = int(R.reject(keys, ml.item_count, rows, out.reshape(-1)).sum())
    print(f"ml-small: {false_neg} false negatives of {len(rows)}, E = {E:.3e}")
    assert false_neg <= 3 + 10 * E


def _chi2_quantile(df, q_tail=1e-6):
    from scipy.stats import chi2

    return float(chi2.isf(q_tail, df))


def test_sampler_distribution(ml, gpu):
    "2^20 draws for one light user: uniform over its negatives; popular ~ the item counts"
    from lkpy_amd import _device as D

    n_items = ml.item_count
    lens = np.diff(ml._indptr)
    u = int(np.flatnonzero(lens == lens[lens > 0].min())[0])
    own = ml._cols[ml._indptr[u]:ml._indptr[u + 1]]
    dp, dc = _dev_csr(ml._indptr, ml._cols, gpu)
    rows = np.full(1 << 20, u, np.int32)
    bins = (np.arange(n_items) * 64) // n_items
    for weighting in ("uniform", "popular"):
        out = D.flexmf_sample_negatives(dp, dc, n_items, rows, 1, weighting, 77, 1)
        out = out.cpu().numpy().reshape(-1)
        assert not np.isin(out, own).any()  # (a light user: c^11 is nothing)
        mass = np.ones(n_items) if weighting == "uniform" else \
            np.bincount(ml._cols, minlength=n_items).astype(np.float64)
        mass[own] = 0.0  # rejection renormalises over the user's negatives
        expect = np.bincount(bins, weights=mass, minlength=64) / mass.sum() * len(out)
        got = np.bincount(bins[out], minlength=64)
        stat = float(((got - expect) ** 2 / expect).sum())
        print(f"{weighting}: chi-square {stat:.1f} on 63 degrees of freedom")
        assert stat < _chi2_quantile(63)


def test_sampler_is_a_function_of_key_and_counter(ml, gpu):
    from lkpy_amd import _device as D

    dp, dc = _dev_csr(ml._indptr, ml._cols, gpu)
    rows = ml._rows[:50000]
    a = D.flexmf_sample_negatives(dp, dc, ml.item_count, rows, 2, "uniform", 11, 3).cpu().numpy()
    b = D.flexmf_sample_negatives(dp, dc, ml.item_count, rows, 2, "uniform", 11, 3).cpu().numpy()
    c = D.flexmf_sample_negatives(dp, dc, ml.item_count, rows, 2, "uniform", 12, 3).cpu().numpy()
    d = D.flexmf_sample_negatives(dp, dc, ml.item_count, rows, 2, "uniform", 11, 4).cpu().numpy()
    assert np.array_equal(a, b)
    assert (a != c).mean() > 0.99 and (a != d).mean() > 0.99


def test_matrix_sample_negatives(ml, gpu):
    m = ml.interactions().matrix()
    rows = ml._rows[:1000]
    one = m.sample_negatives(rows, rng=np.random.default_rng(0))
    assert one.shape == (1000,) and one.dtype == np.int32
    many = m.sample_negatives(rows, n=4, weighting="popular", rng=np.random.default_rng(0))
    assert many.shape == (1000, 4) and many.dtype == np.int32
    assert one.min() >= 0 and many.max() < ml.item_count
    again = m.sample_negatives(rows, rng=np.random.default_rng(0))
    assert np.array_equal(one, again)
    with pytest.raises(ValueError):
        m.sample_negatives(rows, weighting="nonesuch")


# ---- WARP search ----------------------------------------------------------------------------
def _warp_case(ml):
    tabs = _init(ml, 64, False, True, seed=4)
    rng = np.random.default_rng(6)
    # a spread-out model, so that scores are not all within rounding of each other
    for name in ("u_embed.weight", "i_embed.weight"):
        tabs[name] = (tabs[name] * 5.0).astype(np.float32)
    sel = rng.permutation(len(ml._rows))[:4096]
    users, pos = ml._rows[sel], ml._cols[sel]
    cand = rng.integers(0, ml.item_count, (len(sel), R.MAX_TRIES)).astype(np.int32)
    P, Q, bi = tabs["u_embed.weight"], tabs["i_embed.weight"], tabs["i_bias.weight"].reshape(-1)
    sp = bi[pos] + np.einsum("bk,bk->b", P[users], Q[pos])
    sc = bi[cand] + np.einsum("bk,btk->bt", P[users], Q[cand])
    return tabs, users, pos, cand, sp.astype(np.float32), sc.astype(np.float32)


def test_warp_table_margin_on_the_cpu(ml):
    "the table leaves at most 1 % of the samples within 1e-5 of a decision (restatement alone)"
    _, _, _, cand, sp, sc = _warp_case(ml)
    _, _, margin = R.warp_search_sequential(sp, cand, sc)
    assert (margin < 1e-5).mean() <= 0.01


def test_warp_search(ml, gpu):
    tabs, users, pos, cand, sp, sc = _warp_case(ml)
    items, counts, margin = R.warp_search_sequential(sp, cand, sc)
    keep = margin >= 1e-5
    assert (~keep).mean() <= 0.01
    st = _device_state(tabs, gpu, loss="warp", reg_method="AdamW")
    neg, cnt, w = (t.cpu().numpy() for t in st.warp_search(users, pos, cand))
    print(f"WARP search: {int((~keep).sum())} of {len(keep)} samples left out; counts "
          f"{counts.min()} .. {counts.max()}, never found: {int((counts == 200).sum())}")
    assert np.array_equal(neg[keep], items[keep]) and np.array_equal(cnt[keep], counts[keep])
    want = R.warp_weights(counts, ml.item_count)
    assert np.abs(w[keep] / want[keep] - 1.0).max() <= 1e-12


# ---- component ------------------------------------------------------------------------------
EXTRA_USERS = [900001, 900002]  # known to the vocabulary, no interactions


@pytest.fixture(scope="module")
def ml_plus(ml):
    from lkpy_amd.data import Dataset, Vocabulary

    users = Vocabulary(np.concatenate([ml.users.ids(), EXTRA_USERS]), "user")
    return Dataset(users, ml.items, users.numbers(ml.users.ids(ml._rows)), ml._cols, ml._attrs)


@pytest.fixture(scope="module")
def trained(ml_plus, gpu):
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.training import TrainingOptions

    out = {}
    for name in PRESET_TOMLS:
        pipe = Pipeline.load_config(GOLDEN / "pipelines" / f"{name}.toml")
        pipe.train(ml_plus, TrainingOptions(rng=13))
        out[name] = pipe
    return out


@pytest.mark.parametrize("name", PRESET_TOMLS)
def test_component(ml_plus, gpu, trained, name):
    ml = ml_plus
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.flexmf import FlexMFImplicitScorer

    pipe = trained[name]
    sc = pipe.node("scorer").component
    assert isinstance(sc, FlexMFImplicitScorer) and sc.is_trained() and sc.trained_epochs == 10
    cfg = sc.config
    P, Q = sc.user_embeddings, sc.item_embeddings
    assert P.shape == (ml.user_count, 64) and Q.shape == (ml.item_count, 64)
    assert P.dtype == np.float32 and np.isfinite(P).all() and np.isfinite(Q).all()
    assert (sc.user_bias is None) == (not cfg.selected_user_bias())
    assert (sc.item_bias is None) == (not cfg.item_bias)
    if sc.item_bias is not None:
        assert sc.item_bias.shape == (ml.item_count,)
    if sc.user_bias is not None:
        assert sc.user_bias.shape == (ml.user_count,)
    # users without interactions stay exactly zero under AdamW (no gradient, decay of zero)
    empty = ml.users.numbers(np.asarray(EXTRA_USERS))
    assert (np.diff(ml._indptr)[empty] == 0).all() and not P[empty].any()
    assert sc.user_bias is None or not sc.user_bias[empty].any()
    assert P[np.diff(ml._indptr) > 0].any(axis=1).all()

    items = ItemList(item_ids=np.concatenate([ml.items.ids()[:300], [-5, -6]]))
    uid = ml.users.ids()[17]
    got = sc(uid, items).scores()
    assert np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()
    bu = 0.0 if sc.user_bias is None else sc.user_bias[17]
    bi = 0.0 if sc.item_bias is None else sc.item_bias[:300]
    want = bu + bi + Q[:300].astype(np.float64) @ P[17].astype(np.float64)
    # per element, 1e-5 relative to the size of what is summed (a score may cancel to near 0)
    size = np.abs(bu) + np.abs(bi) + np.abs(Q[:300]).astype(np.float64) @ np.abs(P[17])
    assert (np.abs(got[:-2] - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    assert np.isnan(sc(-12345, items).scores()).all()  # an unknown user: no fold-in
    assert np.isnan(sc(None, items).scores()).all()

    # recommend_batch = the top n of the per-query scores with the history removed, same bits
    lookup = pipe.node("history-lookup").component
    uids = np.concatenate([ml.users.ids()[[3, 17, 99, 400]], [-777]])
    hb = lookup.batch(uids)
    idx, val = sc.recommend_batch(hb, 10)
    assert idx.shape == (5, 10) and (idx[4] == -1).all() and np.isnan(val[4]).all()
    all_items = ItemList.from_vocabulary(ml.items)
    for r, u in enumerate(uids[:4]):
        s = sc(u, all_items).scores().copy()
        un = ml.users.number(u)
        s[ml._cols[ml._indptr[un]:ml._indptr[un + 1]]] = -np.inf
        assert np.array_equal(val[r].view(np.uint32), s[idx[r]].view(np.uint32))
        kth = np.sort(s)[::-1][:10]
        assert np.array_equal(val[r].view(np.uint32), kth.view(np.uint32))
    i2, v2 = sc.recommend_batch([lookup(RecQuery.create(u.item())) for u in uids], 10)
    assert np.array_equal(i2, idx) and np.array_equal(v2.view(np.uint32), val.view(np.uint32))

    # batch.recommend routes the id array to the array path
    calls = []
    orig = sc.recommend_batch
    sc.recommend_batch = lambda q, n, **kw: (calls.append(type(q).__name__), orig(q, n, **kw))[1]
    try:
        recs = batch.recommend(pipe, uids[:4], 10)
    finally:
        del sc.recommend_batch
    assert calls == ["HistoryBatch"]
    assert np.array_equal(recs.lookup(uids[1]).numbers(vocabulary=ml.items), idx[1])

    # a pickle round trip scores within the reference's contract (1e-3) and holds no device state
    blob = pickle.dumps(sc)
    sc2 = pickle.loads(blob)
    assert "_dev" not in sc2.__dict__ and "_pending_sync" not in sc2.__dict__
    assert np.abs(sc2(uid, items).scores()[:-2] - got[:-2]).max() <= 1e-3


def test_retrain_false_skips(ml_plus, gpu, trained):
    ml = ml_plus
    from lkpy_amd.training import TrainingOptions

    sc = trained["flexmf-bpr"].node("scorer").component
    before = sc.item_embeddings
    sc.train(ml, TrainingOptions(retrain=False, rng=99))
    assert sc.item_embeddings is before


def test_seeds(ml, gpu):
    from lkpy_amd.flexmf import FlexMFImplicitScorer
    from lkpy_amd.training import TrainingOptions

    def fit(seed):
        sc = FlexMFImplicitScorer(preset="bpr", epochs=2)
        sc.train(ml, TrainingOptions(rng=seed))
        return sc

    a, b, c = fit(5), fit(5), fit(6)
    assert np.array_equal(a.user_embeddings.view(np.uint32), b.user_embeddings.view(np.uint32))
    assert np.array_equal(a.item_embeddings.view(np.uint32), b.item_embeddings.view(np.uint32))
    assert not np.array_equal(a.item_embeddings, c.item_embeddings)


def test_trainer_parameters_and_epoch_loss(ml, gpu):
    from lkpy_amd.flexmf import FlexMFImplicitScorer
    from lkpy_amd.training import TrainingOptions

    sc = FlexMFImplicitScorer(epochs=1)
    tr = sc.create_trainer(ml, TrainingOptions(rng=2))
    # the reference's initial parameters bit for bit from the same seed
    want = _init(ml, 64, True, True, seed=2)
    p0 = tr.get_parameters()
    assert set(p0) == set(R.TABLES)
    for name in R.TABLES:
        assert np.array_equal(p0[name], want[name]), name
    first = tr.train_epoch()["loss"]
    second = tr.train_epoch()["loss"]
    assert 0.0 < second < first < 1.0  # logistic loss falls from about log 2
    p2 = tr.get_parameters()
    tr.load_parameters(p0)
    assert np.array_equal(sc.item_embeddings, want["i_embed.weight"])
    tr.load_parameters(p2)
    assert np.array_equal(sc.user_bias, p2["u_bias.weight"].reshape(-1))


def test_lightgcn_raises(ml, gpu):
    from lkpy_amd.flexmf import FlexMFImplicitScorer

    with pytest.raises(NotImplementedError, match="LightGCN"):
        FlexMFImplicitScorer(preset="lightgcn").train(ml)


def test_largest_embedding_size(ml, gpu):
    "k = 256, the configuration's limit: four registers per lane in training, 258 columns in scoring"
    from lkpy_amd.data import ItemList
    from lkpy_amd.flexmf import FlexMFImplicitScorer
    from lkpy_amd.training import TrainingOptions

    sc = FlexMFImplicitScorer(embedding_size_exp=8, epochs=1)
    tr = sc.create_trainer(ml, TrainingOptions(rng=4))
    p0 = tr.get_parameters()
    users, pos = ml._rows[:4096], ml._cols[:4096]
    neg = np.random.default_rng(0).integers(0, ml.item_count, (4096, 1)).astype(np.int32)
    kw = dict(loss="logistic", reg_method="AdamW", regularization=0.01, learning_rate=0.01,
              negative_count=1, positive_weight=1.0)
    _parity(p0, [(users, pos, neg, None)] * 3, gpu, "k=256", **kw)
    sc.train(ml, TrainingOptions(rng=4))
    P, Q = sc.user_embeddings, sc.item_embeddings
    assert P.shape == (ml.user_count, 256) and Q.shape == (ml.item_count, 256)
    got = sc(ml.users.ids()[5], ItemList(item_ids=ml.items.ids()[:200])).scores()
    want = sc.user_bias[5] + sc.item_bias[:200] + Q[:200].astype(np.float64) @ P[5]
    size = np.abs(sc.user_bias[5]) + np.abs(sc.item_bias[:200]) + np.abs(Q[:200]).astype(np.float64) @ np.abs(P[5])
    assert (np.abs(got - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    idx, val = sc.recommend_batch([ml.users.ids()[5].item()], 5, exclude_history=False)
    full = sc(ml.users.ids()[5], ItemList.from_vocabulary(ml.items)).scores()
    assert np.array_equal(val[0].view(np.uint32), np.sort(full)[::-1][:5].view(np.uint32))


# ---- quality --------------------------------------------------------------------------------
QUALITY_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("preset", ["bpr", "logistic", "warp"])
def test_quality(ml, gpu, preset):
    """quick_measure_model NDCG against the Torch restatement trainer's five CPU runs
    (tests/golden/flexmf_quality.json): at least their lowest minus their range -- the sampling
    streams differ and the restatement itself spreads from seed to seed -- and above the
    reference's own sanity floor of 0.01.

    ``quick_measure_model`` trains without a seed, and a device run spreads from seed to seed as a
    restatement run does (BPR: 0.1525 .. 0.1738 over four runs, floor 0.1514), so a single
    unseeded run would make this test a coin that sometimes lands on the wrong side.  The model is
    therefore trained from each of three fixed seeds, chosen before any was run; every one of the
    three runs is held to the floor, and so is their mean (which a shifted trainer would miss even
    if single runs scraped past).  The runs are the same on every machine."""
    from dataclasses import replace

    from lkpy_amd.flexmf import FlexMFImplicitScorer
    from lkpy_amd.metrics import quick_measure_model
    from lkpy_amd.training import TrainingOptions

    gold = json.loads((GOLDEN / "flexmf_quality.json").read_text())
    ref = np.asarray(gold["ndcg"][preset])
    floor = ref.min() - (ref.max() - ref.min())
    vals = []
    for seed in QUALITY_SEEDS:
        class Seeded(FlexMFImplicitScorer):
            def train(self, data, options=TrainingOptions(), _seed=seed):
                super().train(data, replace(options, rng=_seed))

        res = quick_measure_model(Seeded(preset=preset), ml, rng=gold["split_seed"])
        vals.append(float(res.list_summary().loc["NDCG", "mean"]))
    print(f"{preset}: NDCG {[round(v, 4) for v in vals]}, mean {np.mean(vals):.4f}; restatement "
          f"{ref.min():.4f} .. {ref.max():.4f} (mean {ref.mean():.4f}), floor {floor:.4f}")
    assert min(vals) >= floor  # each device run reaches the lowest of the five minus their range
    assert np.mean(vals) >= floor
    assert min(vals) > 0.01
