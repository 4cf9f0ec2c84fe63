"""
The randomized SVD trainer on the device (csrc/svd.hip, ``lkpy_amd._device.randomized_svd``) and
``lkpy_amd.sklearn.svd.BiasedSVDScorer``.

Bars.  ``lk_csr_spmm``: per cell ``|err| <= (len + 2) 2^-24 sum |val x|`` against the float64
product: a term of a row of ``len`` entries passes through at most ``len`` roundings (its
segment's chain of fused multiply-adds and the additions of the segment sums, which are fewer
than the chain links they replace).  ``lk_chol_upper_inverse`` and the orthonormalisation: 4 x
the residual of the float32 library routine (``numpy.linalg.cholesky``, ``scipy.linalg.qr``) on
the same input.  ``randomized_svd`` and the scorer: 4 x the distance of the float32 NumPy
restatement (``tests/svd_restatement.py``) from its float64 run, computed here from the same
inputs -- the convention of ``tests/test_gpu_flexmf.py``.
"""
import pickle
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sps
import torch

import svd_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
U24 = 2.0 ** -24


def _dev_csr(mat, gpu, is64):
    from lkpy_amd import _device as D

    ptr = mat.indptr.astype(np.int64 if is64 else np.int32)
    return D.DeviceCSR.from_arrays(ptr, mat.indices, mat.data, mat.shape, gpu)


def _panel(x, l, gpu, pad=0.0):
    "host [n x l] -> the padded device panel; ``pad`` is what the pad columns hold"
    from lkpy_amd import _device as D

    p = D.to_device_padded(np.ascontiguousarray(x, np.float32), gpu)
    if pad:
        p[:, l:] = pad
    return p


# ---- lk_csr_spmm ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_matrix():
    """40 x 50 random rows, then rows of 0, 1, split - 1, split, split + 1 and 3 split + 5
    entries with repeated column indices in entry order; the longest row is the last"""
    from lkpy_amd import _device as D

    split = D.spmm_split()
    assert split == 256
    rng = np.random.default_rng(11)
    base = sps.random_array((40, 50), density=0.3, rng=rng, dtype=np.float32).tocsr()
    base.sort_indices()
    lens = [0, 1, split - 1, split, split + 1, 3 * split + 5]
    idx = [rng.integers(0, 50, n).astype(np.int32) for n in lens]
    val = [rng.normal(size=n).astype(np.float32) for n in lens]
    ptr = np.concatenate([base.indptr, base.indptr[-1] + np.cumsum(lens)])
    mat = sps.csr_array((np.concatenate([base.data, *val]),
                         np.concatenate([base.indices, *idx]), ptr), shape=(46, 50))
    assert len(np.unique(idx[2])) < len(idx[2]) and (np.diff(idx[2]) < 0).any()  # repeats, unsorted
    return mat, lens


def _spmm_check(mat, l, gpu, is64):
    from lkpy_amd import _device as D

    rng = np.random.default_rng(l)
    x = rng.normal(size=(mat.shape[1], l)).astype(np.float32)
    got_dev = D.csr_spmm(_dev_csr(mat, gpu, is64), _panel(x, l, gpu, pad=3.0), l)
    assert tuple(got_dev.shape) == (mat.shape[0], D.padded_dim(l))
    got = got_dev.cpu().numpy()
    assert not got[:, l:].any()  # pad columns are written, as zero
    # (copies: SciPy may put a matrix it multiplies into canonical order in place)
    a64 = sps.csr_array((mat.data.astype(np.float64), mat.indices.copy(), mat.indptr.copy()),
                        shape=mat.shape)
    want = a64 @ x.astype(np.float64)
    size = abs(a64) @ np.abs(x.astype(np.float64))
    lens = np.diff(mat.indptr)
    bound = ((lens + 2) * U24)[:, None] * size
    err = np.abs(got[:, :l] - want)
    assert (err <= bound).all(), (l, float((err - bound).max()))
    assert not got[lens == 0].any()
    return got


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("l", [1, 11, 18, 74, 138, 300, 700, 1000])
def test_spmm_edges(edge_matrix, gpu, l, is64):
    from lkpy_amd import _device as D

    mat, lens = edge_matrix
    entry_order = mat.indices.copy()
    got = _spmm_check(mat, l, gpu, is64)
    assert np.array_equal(mat.indices, entry_order)
    # a row alone gives the bits it has inside the matrix
    rng = np.random.default_rng(l)
    x = _panel(rng.normal(size=(50, l)).astype(np.float32), l, gpu, pad=3.0)
    for r in (3, 39, 41, 42, 43, 44, 45):
        lo, hi = mat.indptr[r], mat.indptr[r + 1]
        one = sps.csr_array((mat.data[lo:hi], mat.indices[lo:hi], [0, hi - lo]), shape=(1, 50))
        alone = D.csr_spmm(_dev_csr(one, gpu, is64), x, l).cpu().numpy()
        assert np.array_equal(alone.view(np.uint32), got[r:r + 1].view(np.uint32)), (l, r)


def test_spmm_many_blocks_and_bad_indices(gpu):
    "more rows than one workgroup holds, and an index that is no row of the panel adds nothing"
    from lkpy_amd import _device as D

    rng = np.random.default_rng(5)
    mat = sps.random_array((1003, 77), density=0.05, rng=rng, dtype=np.float32).tocsr()
    _spmm_check(mat, 18, gpu, False)
    bad = mat.copy()
    bad.indices = bad.indices.copy()
    hit = rng.random(bad.nnz) < 0.1
    bad.indices[hit] = np.where(rng.random(int(hit.sum())) < 0.5, -1, 77)
    keep = mat.copy()
    keep.data = np.where(hit, 0.0, keep.data).astype(np.float32)
    x = _panel(rng.normal(size=(77, 18)).astype(np.float32), 18, gpu)
    got = D.csr_spmm(_dev_csr(bad, gpu, False), x, 18).cpu().numpy()
    want = D.csr_spmm(_dev_csr(keep, gpu, False), x, 18).cpu().numpy()
    assert np.array_equal(got, want)


# ---- lk_chol_upper_inverse --------------------------------------------------------------------
def _gram(l, seed, rows=500):
    y = np.random.default_rng(seed).normal(size=(rows, l))
    return (y.T @ y).astype(np.float32)


def _inverse_residual(t, g):
    "|| R^-T G R^-1 - I ||max in float64, T = (R^-1)^T"
    t = t.astype(np.float64)
    return float(np.abs(t @ g.astype(np.float64) @ t.T - np.eye(len(g))).max())


@pytest.mark.parametrize("l", [1, 11, 74, 138, 192, 200])
def test_chol_upper_inverse(gpu, l):
    "(l = 200 is beyond the kernel's LDS: the library path of the same call)"
    from lkpy_amd import _device as D

    assert D.chol_max_l() == 192
    g = _gram(l, l)
    low_np = np.linalg.cholesky(g)
    assert low_np.dtype == np.float32
    t_np = sla.solve_triangular(low_np, np.eye(l, dtype=np.float32), lower=True)
    ref = _inverse_residual(t_np, g)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    inv, low = D.chol_upper_inverse(torch.from_numpy(g).to(gpu), flag, 7, want_lower=True)
    ld = D.padded_dim(l)
    assert tuple(inv.shape) == (ld, ld) and tuple(low.shape) == (ld, ld)
    inv, low = inv.cpu().numpy(), low.cpu().numpy()
    assert int(flag.item()) == 0
    for m in (inv, low):  # lower triangular inside l x l, zero pads
        assert not np.triu(m[:l, :l], 1).any() and not m[l:].any() and not m[:, l:].any()
    got = _inverse_residual(inv[:l, :l], g)
    fac = np.abs(low[:l, :l].astype(np.float64) @ low[:l, :l].T - g).max() / np.abs(g).max()
    fac_np = np.abs(low_np.astype(np.float64) @ low_np.T - g).max() / np.abs(g).max()
    print(f"l={l}: inverse residual device {got:.2e}, numpy float32 {ref:.2e}; factor residual "
          f"device {fac:.2e}, numpy {fac_np:.2e}")
    assert got <= 4.0 * ref
    assert fac <= 4.0 * max(fac_np, U24)


@pytest.mark.parametrize("l", [11, 74, 200])
def test_chol_flags_a_singular_gramian(gpu, l):
    from lkpy_amd import _device as D

    y = np.random.default_rng(l).normal(size=(500, l))
    y[:, l - 2] = y[:, 0] + y[:, 1]  # an exactly dependent column
    y[:, l - 1] = y[:, 0]
    g = (y.T @ y).astype(np.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    inv, low = D.chol_upper_inverse(torch.from_numpy(g).to(gpu), flag, 5, want_lower=True)
    assert int(flag.item()) == 5
    assert torch.isfinite(inv).all() and torch.isfinite(low).all()
    # the first failing step stays in the flag
    D.chol_upper_inverse(torch.from_numpy(g).to(gpu), flag, 9)
    assert int(flag.item()) == 5


# ---- orthonormalisation -----------------------------------------------------------------------
def _conditioned_panel(rows, l, cond, seed):
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.normal(size=(rows, l)))
    v, _ = np.linalg.qr(rng.normal(size=(l, l)))
    s = np.logspace(0, -np.log10(cond), l) if l > 1 else np.ones(1)
    return ((u * s) @ v.T).astype(np.float32)


def _orth_quality(q, y):
    q, y = q.astype(np.float64), y.astype(np.float64)
    return (float(np.abs(q.T @ q - np.eye(q.shape[1])).max()),
            float(np.linalg.norm(y - q @ (q.T @ y)) / np.linalg.norm(y)))


@pytest.mark.parametrize("l,cond", [(1, 1), (18, 1), (18, 1e2), (18, 1e3), (74, 1), (74, 1e2),
                                    (74, 1e3), (138, 1e3), (200, 1e2)])
def test_cholesky_qr2(gpu, l, cond):
    from lkpy_amd import _device as D

    y = _conditioned_panel(500, l, cond, 100 + l)
    q_ref, _ = sla.qr(y, mode="economic")
    assert q_ref.dtype == np.float32
    ref = _orth_quality(q_ref, y)
    orth = D.CholeskyQR2(l, gpu)
    q_dev, rt = orth(_panel(y, l, gpu), "test panel", keep_factor=True)
    assert orth.failed_step() is None
    q = q_dev.cpu().numpy()
    assert not q[:, l:].any()
    got = _orth_quality(q[:, :l], y)
    r = rt.cpu().numpy()[:l, :l].T.astype(np.float64)  # Y = Q R
    back = float(np.linalg.norm(q[:, :l].astype(np.float64) @ r - y) / np.linalg.norm(y))
    print(f"l={l} cond={cond:g}: |Q^T Q - I| device {got[0]:.2e} scipy {ref[0]:.2e}; "
          f"|Y - Q Q^T Y|/|Y| device {got[1]:.2e} scipy {ref[1]:.2e}; |Q R - Y|/|Y| {back:.2e}")
    assert got[0] <= 4.0 * ref[0]
    assert got[1] <= 4.0 * ref[1]
    # Y R1^-1, Q1 R2^-1, R2 R1 and the substitution behind each inverse are chains of at most l
    # fused multiply-adds; undoing R1^-1 by R1 magnifies its rounding by at most cond(R1) = cond
    assert np.allclose(np.triu(r), r) and back <= 4 * l * U24 * cond


# ---- D.randomized_svd -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "svd_ref.npz")


@pytest.fixture(scope="module")
def model(ml):
    return R.bias_residuals(ml._rows, ml._cols, ml._attrs["rating"],
                            (ml.user_count, ml.item_count), 5.0)


@pytest.fixture(scope="module")
def restated(model, gold):
    "{(k, transposed input): (float64 fit, float32 fit)} from the stored start panel, made once"
    out = {}
    for k in (8, 64):
        omega = gold["omega"][:, :k + R.OVERSAMPLES]
        for flipped in (False, True):
            a = sps.csr_array(model[3].T) if flipped else model[3]
            out[k, flipped] = tuple(R.randomized_svd(a, k, 5, omega, dt)
                                    for dt in (np.float64, np.float32))
    return out


def _fit_distance(fit, ref, rows, cols):
    "(singular values, the reconstruction X_t components_ at the sampled cells) max distances"
    s, comp, xt = (np.asarray(a, np.float64) for a in fit)
    s0, comp0, xt0 = ref
    rec = np.einsum("nk,kn->n", xt[rows], comp[:, cols])
    rec0 = np.einsum("nk,kn->n", xt0[rows], comp0[:, cols])
    return float(np.abs(s - s0).max()), float(np.abs(rec - rec0).max())


@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("k", [8, 64])
def test_randomized_svd_parity(gpu, model, gold, restated, k, flipped):
    from lkpy_amd import _device as D

    a = sps.csr_array(model[3].T) if flipped else model[3]
    a.sort_indices()
    csr = _dev_csr(a, gpu, False)
    csr_t = D.csr_transpose(csr)
    omega = gold["omega"][:, :k + R.OVERSAMPLES]
    s, comp, xt = D.randomized_svd(csr, csr_t, k, 5, omega)
    assert s.shape == (k,) and comp.shape == (k, a.shape[1]) and xt.shape == (a.shape[0], k)
    assert comp.dtype == np.float32 and xt.dtype == np.float32
    assert np.isfinite(comp).all() and np.isfinite(xt).all()
    top = comp[np.arange(k), np.abs(comp).argmax(axis=1)]
    assert (top > 0).all()  # svd_flip(u_based_decision=False)
    rng = np.random.default_rng(k)
    rows, cols = rng.integers(0, a.shape[0], 2000), rng.integers(0, a.shape[1], 2000)
    f64, f32 = restated[k, flipped]
    ds32, dr32 = _fit_distance(f32, f64, rows, cols)
    ds, dr = _fit_distance((s, comp, xt), f64, rows, cols)
    print(f"k={k} transposed input={flipped}: singular values device {ds:.2e} float32 "
          f"restatement {ds32:.2e}; reconstruction device {dr:.2e} restatement {dr32:.2e}")
    assert ds32 > 0 and dr32 > 0
    assert ds <= 4.0 * ds32
    assert dr <= 4.0 * dr32
    # device_output: the same factors as padded panels
    s2, v, xt_dev = D.randomized_svd(csr, csr_t, k, 5, omega, device_output=True)
    assert np.array_equal(s2, s) and v.is_cuda
    assert np.array_equal(v.cpu().numpy()[:, :k].T, comp)
    assert np.array_equal(xt_dev.cpu().numpy()[:, :k], xt)


def test_randomized_svd_preconditions(gpu):
    from lkpy_amd import _device as D

    rng = np.random.default_rng(2)
    a = sps.random_array((30, 40), density=0.5, rng=rng, dtype=np.float32).tocsr()
    csr = _dev_csr(a, gpu, False)
    csr_t = D.csr_transpose(csr)
    with pytest.raises(ValueError, match="sketch columns"):
        D.randomized_svd(csr, csr_t, 21, 2, rng.normal(size=(30, 31)))
    with pytest.raises(ValueError, match="omega"):
        D.randomized_svd(csr, csr_t, 8, 2, rng.normal(size=(40, 18)))
    s, comp, xt = D.randomized_svd(csr, csr_t, 20, 2, rng.normal(size=(30, 30)))  # l = min(shape)
    want = np.linalg.svd(a.toarray().astype(np.float64), compute_uv=False)[:20]
    assert np.abs(s - want).max() <= 1e-4 * want[0]


def test_rank_deficient_sketch_raises(gpu):
    "a rank-5 matrix cannot carry an 18-column sketch: RuntimeError naming the step, never NaNs"
    from lkpy_amd import _device as D

    rng = np.random.default_rng(3)
    dense = (rng.normal(size=(30, 5)) @ rng.normal(size=(5, 40))).astype(np.float32)
    csr = _dev_csr(sps.csr_array(dense), gpu, False)
    csr_t = D.csr_transpose(csr)
    with pytest.raises(RuntimeError, match="rank-deficient.*CholeskyQR pass"):
        D.randomized_svd(csr, csr_t, 8, 2, rng.normal(size=(30, 18)))


# ---- the component ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ml, gpu, gold):
    "k = 8 from the stored start panel (injected through the trainer's test hook)"
    from lkpy_amd.sklearn.svd import BiasedSVDScorer

    sc = BiasedSVDScorer(features=8)
    sc._start_panel = gold["omega"][:, :18]
    sc.train(ml)
    return sc


def test_component_state(ml, model, trained):
    sc = trained
    assert sc.is_trained() and sc.users is ml.users and sc.items is ml.items
    assert sc.user_components.shape == (ml.user_count, 8)
    assert sc.user_components.dtype == np.float32
    f = sc.factorization
    assert f.components_.shape == (8, ml.item_count) and f.n_components == 8
    assert f.singular_values_.shape == (8,) and (np.diff(f.singular_values_) <= 0).all()
    x = sc.user_components[:3]
    assert np.array_equal(f.inverse_transform(x), x @ f.components_)
    assert sc.bias.global_bias == model[0] and np.array_equal(sc.bias.user_biases, model[2])


def test_seeded_fits_are_identical(ml, gpu):
    from lkpy_amd.sklearn.svd import BiasedSVDScorer
    from lkpy_amd.training import TrainingOptions

    fits = []
    for _ in range(2):
        sc = BiasedSVDScorer(features=8)
        sc.train(ml, TrainingOptions(rng=7))
        fits.append(sc)
    a, b = fits
    assert np.array_equal(a.user_components.view(np.uint32), b.user_components.view(np.uint32))
    assert np.array_equal(a.factorization.item_factors.view(np.uint32),
                          b.factorization.item_factors.view(np.uint32))
    assert np.array_equal(a.factorization.singular_values_, b.factorization.singular_values_)
    other = BiasedSVDScorer(features=8)
    other.train(ml, TrainingOptions(rng=8))
    assert not np.array_equal(other.user_components, a.user_components)
    before = a.user_components
    a.train(ml, TrainingOptions(rng=9, retrain=False))
    assert a.user_components is before


def test_call_matches_golden_scores(ml, model, gold, restated, trained):
    from lkpy_amd.data import ItemList

    g, ib, ub, _ = model
    _, comp32, xt32 = restated[8, False][1]
    worst, worst32 = 0.0, 0.0
    for r, (u, items) in enumerate(zip(gold["score_users"], gold["score_items"])):
        want = gold["scores_8"][r]
        il = ItemList(item_ids=ml.items.ids()[items])
        got = trained(ml.users.ids()[u].item(), il).scores()
        assert got.dtype == np.float32 and got.shape == (30,)
        f32 = R.score(xt32[u], comp32, items, g, ib, ub[u], np.float32)
        worst = max(worst, float(np.abs(got - want).max()))
        worst32 = max(worst32, float(np.abs(f32.astype(np.float64) - want).max()))
    print(f"golden scores: device {worst:.2e}, float32 restatement {worst32:.2e}")
    assert worst32 > 0
    assert worst <= 4.0 * worst32


def test_call_and_score_batch(ml, trained):
    from lkpy_amd.data import ItemList

    sc = trained
    ids = ml.items.ids()
    uids = ml.users.ids()
    lists = [ItemList(item_ids=np.concatenate([ids[5 * i:5 * i + 20 + i], [-5]]))
             for i in range(12)]
    users = [uids[3 * i].item() for i in range(11)] + [-777]
    batch = sc.score_batch(users, lists)
    for u, il, got in zip(users, lists, batch):
        one = sc(u, il).scores()
        assert np.array_equal(one.view(np.uint32), got.scores().view(np.uint32))
        if u == -777:
            assert np.isnan(one).all()  # an unknown user
        else:
            assert np.isnan(one[-1]) and np.isfinite(one[:-1]).all()  # an unknown item
    assert np.isnan(sc(None, lists[0]).scores()).all()


def test_user_bias_follows_the_query(ml, trained):
    """a query with rated history takes its user bias from those ratings
    (``BiasModel.compute_for_items``), one without takes the stored bias"""
    from lkpy_amd.data import ItemList, RecQuery

    sc = trained
    u = 17
    uid = ml.users.ids()[u].item()
    items = np.arange(40, 70)
    il = ItemList(item_ids=ml.items.ids()[items])
    x = sc.user_components[u].astype(np.float64)
    v = sc.factorization.components_[:, items].astype(np.float64)
    base = x @ v + sc.bias.global_bias + sc.bias.item_biases[items]
    # 11 terms in one float32 chain, the global and the user bias rounded to float32 first
    size = np.abs(x) @ np.abs(v) + sc.bias.global_bias + np.abs(sc.bias.item_biases[items]) + 1.0
    plain = sc(uid, il).scores()
    assert (np.abs(plain - (base + sc.bias.user_biases[u])) <= 16 * U24 * size).all()
    hist = ItemList(item_ids=ml.items.ids()[[1, 2, 3]], rating=np.array([5.0, 5.0, 4.5]))
    _, want_ub = sc.bias.compute_for_items(il, uid, hist)
    assert abs(want_ub - sc.bias.user_biases[u]) > 0.05 and abs(want_ub) < 1.0
    got = sc(RecQuery(user_id=uid, user_items=hist), il).scores()
    assert (np.abs(got - (base + want_ub)) <= 16 * U24 * size).all()


def test_pickle_round_trip(ml, trained):
    from lkpy_amd.data import ItemList

    sc = trained
    il = ItemList(item_ids=np.concatenate([ml.items.ids()[:300], [-5]]))
    uid = ml.users.ids()[9].item()
    got = sc(uid, il).scores()
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__
    assert np.array_equal(sc2.user_components, sc.user_components)
    assert np.array_equal(sc2(uid, il).scores().view(np.uint32), got.view(np.uint32))


def test_recommend_batch_is_the_dense_top_n(ml, gpu, trained):
    from lkpy_amd.basic import UserTrainingHistoryLookup

    sc = trained
    lookup = UserTrainingHistoryLookup()
    lookup.train(ml)
    uids = np.concatenate([ml.users.ids()[::13], [-777]])
    hb = lookup.batch(uids)
    idx, val = sc.recommend_batch(hb, 10)
    panel, valid, hist = sc.dense_scores_batch(hb)
    panel = panel.cpu().numpy()
    assert valid[:-1].all() and not valid[-1]
    assert (idx[-1] == -1).all() and np.isnan(val[-1]).all() and np.isnan(panel[-1]).all()
    for r, un in enumerate(hb.user_nums[:-1]):
        own = ml._cols[ml._indptr[un]:ml._indptr[un + 1]]
        row = panel[r].copy()
        row[own] = -np.inf
        want = np.sort(row)[::-1][:10]
        assert np.array_equal(val[r].view(np.uint32), want.view(np.uint32)), r
        assert np.array_equal(row[idx[r]].view(np.uint32), val[r].view(np.uint32))
        assert not np.isin(idx[r], own).any()
    # the batch's user bias is the one the per-query path computes from the same ratings
    qs = [lookup(u.item()) for u in uids[:5]]
    idx_q, val_q = sc.recommend_batch(qs, 10)
    assert np.abs(val_q - val[:5]).max() <= 16 * U24 * np.abs(val[:5]).max() * 4
    dev_idx, dev_val = sc.recommend_batch(hb, 10, exclude_history=False, device_output=True)
    assert dev_idx.is_cuda and tuple(dev_idx.shape) == (len(uids), 10)


def test_pipeline(ml, gpu):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.sklearn.svd import BiasedSVDScorer
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "biased-svd.toml")
    pipe.train(ml, TrainingOptions(rng=21))
    sc = pipe.node("scorer").component
    assert isinstance(sc, BiasedSVDScorer) and sc.factorization.n_components == 64
    uids = ml.users.ids()[:50]
    recs = batch.recommend(pipe, uids, 10)
    for u in uids:
        il = recs.lookup(u)
        assert len(il) == 10 and (np.diff(il.scores()) <= 0).all()
        un = ml.users.number(u)
        assert not np.isin(il.numbers(vocabulary=ml.items),
                           ml._cols[ml._indptr[un]:ml._indptr[un + 1]]).any()
    pairs = {u.item(): ItemList(item_ids=np.concatenate([ml.items.ids()[7 * n:7 * n + 12], [-5]]))
             for n, u in enumerate(uids)}
    preds = batch.predict(pipe, pairs)
    for u, il in pairs.items():
        got = preds.lookup(u)
        assert np.array_equal(got.ids(), il.ids()) and np.isfinite(got.scores()).all()
        one = pipe.run("rating-predictor", query=u, items=il)
        assert np.array_equal(got.scores().view(np.uint32), one.scores().view(np.uint32))


def test_arpack_is_not_implemented(ml, gpu):
    from lkpy_amd.sklearn.svd import BiasedSVDScorer

    sc = BiasedSVDScorer(features=8, algorithm="arpack")
    with pytest.raises(NotImplementedError, match="arpack"):
        sc.train(ml)
    assert not sc.is_trained()
    with pytest.raises(ValueError, match="sketch columns"):
        BiasedSVDScorer(features=700).train(ml)
