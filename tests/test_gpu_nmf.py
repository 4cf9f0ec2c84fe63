"""
NMF on the device (csrc/nmf.hip, ``lkpy_amd._device.nmf_fit``, lkpy_amd/sklearn/nmf.py) against
the NumPy restatement of ``tests/nmf_restatement.py``, which ``tests/test_nmf_host.py`` holds to
scikit-learn.

The sweep kernel promises the restatement's bits and is held to the bit.  A whole fit also goes
through the Gramian and the sparse product, whose sums run in another order, so it is held to the
project's criterion (``tests/test_gpu_lightgcn.py``): the distance of the device from the FLOAT64
restatement is at most 4 x the distance of the FLOAT32 restatement from it, computed in the same
test from the same inputs, and that yardstick must itself be above zero.  Reconstructions ``W H``
are compared, not factors (``tests/test_nmf_host.py``).
"""
import pickle
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import nmf_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
NS = [1, 63, 64, 65, 257, 1003]      # one lane, a wave less one, a wave, one more, 5 and 16 blocks
KS = [1, 5, 16, 17, 64, 100, 128]    # every padded width (16, 32, 64, 128), full and not
UNKNOWN_USER = -777


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- lk_nmf_cd_sweep ------------------------------------------------------------------------------
def _sweep_inputs(n, k, seed):
    """(W [n x k], HHt [k x k], XHt [n x k]) as float32 host arrays: about 30 % exact zeros in W,
    one all-zero column of Ht (a zero Hessian) where k > 1, and where n > 2 one all-zero row of W
    whose row of X -- and so of XHt -- is zero."""
    rng = np.random.default_rng(seed)
    m = 40
    ht = rng.random((m, k)).astype(np.float32)
    if k > 1:
        ht[:, k // 2] = 0
    x = (rng.random((n, m)) < 0.3).astype(np.float32)
    w = rng.random((n, k)).astype(np.float32)
    w[rng.random((n, k)) < 0.3] = 0
    if n > 2:
        w[n // 2] = 0
        x[n // 2] = 0
    return w, (ht.T @ ht).astype(np.float32), (x @ ht).astype(np.float32)


def _device_sweep(gpu, w, hht, xht, l1, ld_h=None):
    from lkpy_amd import _device as D

    k = w.shape[1]
    d_w = D.to_device_padded(w, gpu)
    d_h = torch.from_numpy(hht).to(gpu)
    if ld_h is not None:  # a [k x k] view of a wider matrix
        wide = torch.full((k, ld_h), float("nan"), dtype=torch.float32, device=gpu)
        wide[:, :k] = d_h
        d_h = wide[:, :k]
    viol = D.nmf_cd_sweep(d_w, d_h, D.to_device_padded(xht, gpu), l1)
    got = d_w.cpu().numpy()
    assert got.shape == (len(w), D.padded_dim(k)) and not got[:, k:].any()  # pad columns
    return got[:, :k], float(viol.cpu().numpy()[0])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_sweep_bits(gpu, n, k):
    "every n with every k; l1_reg is 0 where n + k is even and positive where it is odd"
    l1 = 0.0 if (n + k) % 2 == 0 else 0.0625 + 0.01
    w, hht, xht = _sweep_inputs(n, k, 1000 * n + k)
    assert k == 1 or (hht[k // 2] == 0).all()
    got, viol = _device_sweep(gpu, w, hht, xht, l1)
    want = w.copy()
    pg = R.sweep(want, hht, xht, l1)
    if n >= 63:  # the sweep moved entries, and clamped some at zero
        assert (want != w).any() and ((want == 0) & (w != 0)).any() == (k > 1)
    assert np.array_equal(_bits(got), _bits(want))
    v = R.violation(pg)
    assert abs(viol - v) <= 1e-9 * v


@pytest.mark.parametrize("l1", [0.0, 0.3])
def test_sweep_bits_both_l1_and_a_strided_hht(gpu, l1):
    w, hht, xht = _sweep_inputs(257, 17, 7)
    got, viol = _device_sweep(gpu, w, hht, xht, l1, ld_h=23)
    want = w.copy()
    pg = R.sweep(want, hht, xht, l1)
    assert np.array_equal(_bits(got), _bits(want))
    assert abs(viol - R.violation(pg)) <= 1e-9 * R.violation(pg)
    # the zero row with a zero XHt row: with l1_reg = 0 nothing moves and nothing is violated
    if l1 == 0.0:
        assert not got[257 // 2].any() and not pg[257 // 2].any()


def test_sweep_is_repeatable_and_refuses_large_k(gpu):
    from lkpy_amd import _device as D

    w, hht, xht = _sweep_inputs(1003, 64, 3)
    a, va = _device_sweep(gpu, w, hht, xht, 0.01)
    b, vb = _device_sweep(gpu, w, hht, xht, 0.01)
    assert np.array_equal(_bits(a), _bits(b)) and va == vb  # the violation too: a fixed order
    assert D.nmf_max_k() == 128
    k = 129
    with pytest.raises(ValueError, match="lk_nmf_max_k"):
        D.nmf_cd_sweep(torch.zeros((4, D.padded_dim(k)), device=gpu),
                       torch.zeros((k, k), device=gpu),
                       torch.zeros((4, D.padded_dim(k)), device=gpu), 0.0)


# ---- the fit from a given start ------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "nmf_ref.npz")


@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def ml_x(ml):
    x = ml.interactions().matrix().scipy(layout="csr").astype(np.float32)
    x.sort_indices()
    assert x.shape == (671, 9125) and (x.data == 1).all()
    return x


@pytest.fixture(scope="module")
def omega():
    return np.load(GOLDEN / "svd_ref.npz")["omega"]


@pytest.fixture(scope="module")
def starts(ml_x, omega):
    "{(k, dtype name): (W0, H0, (raw W, raw H))} of the restatement from the stored panel"
    return {(k, np.dtype(dt).name): R.start(ml_x, k, omega[:, :k + 10], dt)
            for k in (8, 64) for dt in (np.float32, np.float64)}


def _device_fit(gpu, x, w0, h0, max_iter, tol, regs=(0.0, 0.0, 0.0, 0.0)):
    from lkpy_amd import _device as D

    x = sps.csr_array(x).astype(np.float32)
    x.sort_indices()
    csr = D.DeviceCSR.from_arrays(x.indptr, x.indices, x.data, x.shape, gpu)
    return D.nmf_fit(csr, D.csr_transpose(csr), w0, h0, max_iter, tol, *regs)


def _compare_fit(x, w0, h0, sweeps, regs, got, rows, cols, what):
    "the device fit ``got`` against the restatements run for exactly ``sweeps`` sweeps"
    w, h, n_iter, hist = got
    assert n_iter == sweeps and len(hist) == sweeps
    assert w.dtype == np.float32 and h.dtype == np.float32 and (w >= 0).all() and (h >= 0).all()
    w64, h64, _, hist64 = R.fit(x, w0, h0, sweeps, 0.0, *regs, np.float64)
    w32, h32, _, hist32 = R.fit(x, w0, h0, sweeps, 0.0, *regs, np.float32)
    want = R.recon(w64, h64, rows, cols)
    d32 = np.abs(R.recon(w32, h32, rows, cols) - want).max()
    dev = np.abs(R.recon(w, h, rows, cols) - want).max()
    v32 = np.abs(hist32 / hist64 - 1).max()
    vdev = np.abs(hist / hist64 - 1).max()
    print(f"{what}: reconstruction: float32 {d32:.2e}, device {dev:.2e}; "
          f"violations (relative): float32 {v32:.2e}, device {vdev:.2e}")
    assert d32 > 0 and dev <= 4 * d32
    assert v32 > 0 and vdev <= 4 * v32


@pytest.mark.parametrize("k, sweeps", [(8, 10), (64, 3)])
def test_fit_ml_small(gpu, gold, ml_x, starts, k, sweeps):
    w0, h0 = (gold["ml_w0"], gold["ml_h0"]) if k == 8 else starts[(64, "float32")][:2]
    got = _device_fit(gpu, ml_x, w0, h0, sweeps, 0.0)
    _compare_fit(ml_x, w0, h0, sweeps, (0.0,) * 4, got, gold["ml_rows"], gold["ml_cols"],
                 f"ml_small k={k}, {sweeps} sweeps")


def _regs(gold, name):
    n, m = gold[f"{name}_x"].shape
    a, r = float(gold[f"{name}_alpha_W"]), float(gold[f"{name}_l1_ratio"])
    return m * a * r, n * a * r, m * a * (1 - r), n * a * (1 - r)


@pytest.mark.parametrize("name", ["a", "b"])
def test_fit_stops_by_its_own_ratio(gpu, gold, name):
    "60 x 90, k = 5 and the regularised 200 x 150, k = 16, at the default tol"
    x = gold[f"{name}_x"].astype(np.float32)
    w0, h0, regs = gold[f"{name}_w0"], gold[f"{name}_h0"], _regs(gold, name)
    assert (name == "b") == (regs[0] > 0 and regs[2] > 0)
    got = _device_fit(gpu, x, w0, h0, 200, 1e-4, regs)
    n_iter, hist = got[2], got[3]
    ratio = hist / hist[0]
    print(f"{name}: the device stops after {n_iter} sweeps, sklearn after "
          f"{int(gold[f'{name}_n_iter'])}")
    assert n_iter < 200 and len(hist) == n_iter
    assert int(np.flatnonzero(ratio <= 1e-4)[0]) == n_iter - 1
    rows, cols = np.divmod(np.arange(x.size), x.shape[1])  # every cell
    _compare_fit(x, w0, h0, n_iter, regs, got, rows, cols, name)


def test_fit_stops_at_once_without_violation(gpu):
    """A zero start: both Gramians and both products are zero, so every gradient and every
    Hessian is zero, nothing moves, and the first iteration's violation of 0 ends the fit --
    whatever tol is."""
    x = np.zeros((6, 5), np.float32)
    x[0, 0] = x[3, 2] = 1
    w, h, n_iter, hist = _device_fit(gpu, x, np.zeros((6, 2), np.float32),
                                     np.zeros((2, 5), np.float32), 7, 0.0)
    assert n_iter == 1 and hist.tolist() == [0.0]
    assert not w.any() and not h.any()


# ---- the start ----------------------------------------------------------------------------------
def _scorer(k, omega, **cfg):
    from lkpy_amd.sklearn.nmf import NMFScorer

    sc = NMFScorer(n_components=k, **cfg)
    sc._start_panel = omega[:, :k + 10]
    return sc


@pytest.mark.parametrize("k", [8, 64])
def test_start(gpu, ml_x, omega, starts, k):
    from lkpy_amd import _device as D
    from lkpy_amd.training import TrainingOptions

    csr = D.DeviceCSR.from_arrays(ml_x.indptr, ml_x.indices, ml_x.data, ml_x.shape, gpu)
    w0, h0 = _scorer(k, omega)._start(ml_x, csr, D.csr_transpose(csr), TrainingOptions())
    assert w0.dtype == np.float32 and w0.shape == (671, k) and h0.shape == (k, 9125)
    assert (w0 > 0).all() and (h0 > 0).all()
    w64, h64, raw = starts[(k, "float64")]
    w32, h32, _ = starts[(k, "float32")]
    keep_w, keep_h = ~R.band(raw[0]), ~R.band(raw[1])
    left_out = (~keep_w).sum() + (~keep_h).sum()
    assert left_out <= 1e-3 * (keep_w.size + keep_h.size)
    d32 = max(np.abs(w32 - w64)[keep_w].max(), np.abs(h32 - h64)[keep_h].max())
    dev = max(np.abs(w0 - w64)[keep_w].max(), np.abs(h0 - h64)[keep_h].max())
    print(f"start k={k}: {left_out} cells in the band; float32 {d32:.2e}, device {dev:.2e}")
    assert d32 > 0 and dev <= 4 * d32


def test_end_to_end_loss(gpu, ml, ml_x, omega, starts):
    "k = 8 from the stored panel, 10 sweeps: the loss against the float64 restatement's"
    sc = _scorer(8, omega, epochs=10)
    sc._tol = 0.0
    sc.train(ml)
    assert sc.n_iter_ == 10
    loss = {}
    for name in ("float32", "float64"):
        w0, h0, raw = starts[(8, name)]
        w, h, _, _ = R.fit(ml_x, w0, h0, 10, 0.0, dtype=np.dtype(name).type)
        loss[name] = R.loss(ml_x, w, h)
    # every cell near the threshold forced to the other side of it, in float64
    w0, h0, raw = starts[(8, "float64")]
    avg = np.float64(ml_x.astype(np.float64).mean())
    fw = R.threshold_fill(raw[0], avg, R.band(raw[0]))
    fh = R.threshold_fill(raw[1], avg, R.band(raw[1]))
    w, h, _, _ = R.fit(ml_x, fw, fh, 10, 0.0, dtype=np.float64)
    d_flip = abs(R.loss(ml_x, w, h) - loss["float64"]) / loss["float64"]
    d32 = abs(loss["float32"] - loss["float64"]) / loss["float64"]
    got = R.loss(ml_x, sc.user_components, sc.item_components.T)
    dev = abs(got - loss["float64"]) / loss["float64"]
    print(f"loss {got:.6f}; relative to float64: float32 {d32:.2e}, device {dev:.2e}, "
          f"band cells flipped {d_flip:.2e}")
    assert d32 > 0 and dev <= 4 * d32 + d_flip


# ---- the component --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ml, gpu):
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.sklearn.nmf import NMFScorer
    from lkpy_amd.training import TrainingOptions

    pipe = topn_pipeline(NMFScorer(n_components=8, epochs=5))
    pipe.train(ml, TrainingOptions(rng=13))
    return pipe


def test_seeds(ml, gpu):
    "(a pipeline hands each component a seed spawned from its own: the fits here are direct)"
    from lkpy_amd.sklearn.nmf import NMFScorer
    from lkpy_amd.training import TrainingOptions

    def fit(seed):
        sc = NMFScorer(n_components=8, epochs=5)
        sc.train(ml, TrainingOptions(rng=seed))
        return sc

    a, again, b = fit(13), fit(13), fit(14)
    assert np.array_equal(_bits(a.user_components), _bits(again.user_components))
    assert np.array_equal(_bits(a.item_components), _bits(again.item_components))
    assert not np.array_equal(_bits(a.user_components), _bits(b.user_components))
    # a given start leaves nothing to the generator
    c, d = NMFScorer(n_components=8, epochs=2), NMFScorer(n_components=8, epochs=2)
    for sc, seed in ((c, 1), (d, 2)):
        sc._start_factors = (a.user_components + np.float32(0.01),
                             a.item_components.T + np.float32(0.01))
        sc.train(ml, TrainingOptions(rng=seed))
    assert np.array_equal(_bits(c.user_components), _bits(d.user_components))


def test_component(ml, gpu, trained):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.sklearn.nmf import NMFScorer
    from lkpy_amd.training import TrainingOptions

    ds, pipe = ml, trained
    sc = pipe.node("scorer").component
    assert isinstance(sc, NMFScorer) and sc.is_trained()
    P, Q = sc.user_components, sc.item_components
    assert P.shape == (ds.user_count, 8) and Q.shape == (ds.item_count, 8)
    assert P.dtype == np.float32 and Q.dtype == np.float32
    assert np.isfinite(P).all() and np.isfinite(Q).all() and (P >= 0).all() and (Q >= 0).all()
    assert sc.user_embeddings is P and sc.item_embeddings is Q
    assert sc.user_bias is None and sc.item_bias is None
    assert sc.n_iter_ == 5

    # __call__: NaN for unknown items and unknown users; the history is ignored
    items = ItemList(item_ids=np.concatenate([ds.items.ids()[:300], [-5, -6]]))
    uid = ds.users.ids()[17]
    got = sc(uid, items).scores()
    assert got.dtype == np.float32 and np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()
    want = Q[:300].astype(np.float64) @ P[17].astype(np.float64)
    assert (np.abs(got[:-2] - want) <= 1e-5 * np.abs(want) + 1e-30).all()
    assert np.isnan(sc(UNKNOWN_USER, items).scores()).all()
    assert np.isnan(sc(None, items).scores()).all()
    lists = [ItemList(item_ids=np.concatenate([ds.items.ids()[5 * i:5 * i + 20 + i], [-5]]))
             for i in range(6)]
    users = [ds.users.ids()[3 * i].item() for i in range(5)] + [UNKNOWN_USER]
    for u, il, one in zip(users, lists, sc.score_batch(users, lists)):
        assert np.array_equal(_bits(sc(u, il).scores()), _bits(one.scores()))
        assert np.isnan(one.scores()).all() == (u == UNKNOWN_USER)

    # batch.recommend: the per-query lists, the history excluded, the sorted dense panel
    uids = [int(u) for u in ds.users.ids()[::7][:60]] + [UNKNOWN_USER]
    recs = batch.recommend(pipe, uids, 20)
    assert len(recs) == len(uids)
    for u in uids:
        one = pipe.run("recommender", query=u, n=20)
        il = recs.lookup(u)
        assert np.array_equal(il.ids(), one.ids())
        if len(one):
            assert np.array_equal(_bits(il.scores()), _bits(one.scores()))
    assert len(recs.lookup(UNKNOWN_USER)) == 0
    for u in uids[:10]:
        seen = ds.user_row(u).ids()
        il = recs.lookup(u)
        assert len(il) == 20 and not np.isin(il.ids(), seen).any()
        dense = sc(u, ItemList.from_vocabulary(ds.items)).scores().copy()
        dense[ds.items.numbers(seen)] = -np.inf
        top = np.sort(dense)[::-1][:20]
        assert np.array_equal(_bits(il.scores()), _bits(top))

    # batch.score and batch.predict: the bits of the per-query call
    cand = {u: ItemList(item_ids=np.concatenate([ds.items.ids()[i:i + 40], [-5]]))
            for i, u in enumerate(uids)}
    scored = batch.score(pipe, cand)
    predicted = batch.predict(pipe, cand)
    for u in uids:
        one = sc(u, cand[u]).scores()
        assert np.array_equal(_bits(scored.lookup(u).scores()), _bits(one))
        assert np.array_equal(_bits(predicted.lookup(u).scores()), _bits(one))
        assert np.isnan(one[-1]) and np.isnan(one[:-1]).all() == (u == UNKNOWN_USER)

    # a pickle round trip keeps the factors bit for bit and carries no device state
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__ and sc2.n_iter_ == 5
    assert np.array_equal(_bits(sc2.user_components), _bits(P))
    assert np.array_equal(_bits(sc2.item_components), _bits(Q))
    assert np.array_equal(_bits(sc2(uid, items).scores()[:-2]), _bits(got[:-2]))

    # retrain=False skips
    sc.train(ds, TrainingOptions(retrain=False, rng=99))
    assert sc.item_components is Q and sc.user_components is P


def test_train_refuses_too_many_features(ml, gpu):
    from lkpy_amd.sklearn.nmf import NMFScorer

    from lkpy_amd import _device as D
    from lkpy_amd.training import TrainingOptions

    sc = NMFScorer(n_components=129)
    with pytest.raises(ValueError, match="lk_nmf_max_k"):
        sc.train(ml)
    assert not sc.is_trained()
    # k + 10 sketch columns of the start's SVD need as many rows and columns
    x = sps.random_array((700, 100), density=0.1, rng=np.random.default_rng(0),
                         dtype=np.float32).tocsr()
    x.sort_indices()
    csr = D.DeviceCSR.from_arrays(x.indptr, x.indices, x.data, x.shape, gpu)
    with pytest.raises(ValueError, match="sketch columns"):
        NMFScorer(n_components=96)._start(x, csr, D.csr_transpose(csr), TrainingOptions(rng=1))


def test_pipeline_file(ml, gpu):
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.sklearn.nmf import NMFScorer
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "nmf.toml")
    sc = pipe.node("scorer").component
    assert isinstance(sc, NMFScorer) and sc.config.embedding_size == 8
    pipe.train(ml, TrainingOptions(rng=3))
    assert sc.n_iter_ == 5
    recs = pipe.run("recommender", query=ml.users.ids()[5].item(), n=10)
    assert len(recs) == 10 and np.isfinite(recs.scores()).all()
