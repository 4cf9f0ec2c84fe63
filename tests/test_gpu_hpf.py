"""
Hierarchical Poisson factorization on the device (csrc/hpf.hip, lkpy_amd/hpf.py) against the
NumPy / SciPy restatement of ``tests/hpf_restatement.py``.

What goes through exp, digamma, log and many float32 roundings is held to the project's criterion
(``tests/test_gpu_lightgcn.py``): the distance of the device from the FLOAT64 restatement is at
most 4 x the distance of the FLOAT32 restatement from it, computed in the same test from the same
inputs, and that yardstick must itself be above zero.  What the kernels promise to the bit is
held to the bit.
"""
import pickle
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps
import torch
from scipy.special import digamma

import hpf_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
U24 = 2.0 ** -24
KS = [3, 16, 20, 64, 100, 256]  # groups of 4, 4, 8, 16, 32 and 64 lanes per row
N_USERS, N_ITEMS = 300, 200


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dist(x, want):
    return float(np.abs(np.asarray(x, dtype=np.float64) - want).max())


# ---- the matrices -------------------------------------------------------------------------------
def _counts():
    "300 x 200 Poisson counts from planted Gamma factors: about 22 000 entries, counts up to ~70"
    rng = np.random.default_rng(11)
    theta = rng.gamma(0.2, 2.5, (N_USERS, 6))
    beta = rng.gamma(0.2, 2.5, (N_ITEMS, 6))
    return sps.csr_array(rng.poisson(0.8 * theta @ beta.T).astype(np.float32))


@pytest.fixture(scope="module")
def counts():
    mat = _counts()
    assert 20000 < mat.nnz < 24000 and 50 <= mat.data.max() <= 120
    return mat


def _edge_rows(base, split: int, bad: bool):
    """(indptr, cols, y, shape) of ``base`` with six rows more: none, 1, ``split``, ``split`` + 1
    and 600 entries (columns repeat in the long ones: the kernels take any CSR) and, with
    ``bad``, one column index outside the matrix in the middle of row 7."""
    rng = np.random.default_rng(5)
    n_rows, n_cols = base.shape
    lens = [0, 1, split, split + 1, 600]
    indptr, cols, y = [base.indptr.astype(np.int64)], [base.indices], [base.data]
    for m in lens:
        cols.append(rng.integers(0, n_cols, m).astype(np.int32))
        y.append(rng.integers(1, 9, m).astype(np.float32))
    indptr = np.concatenate([indptr[0], indptr[0][-1] + np.cumsum(lens)])
    cols, y = np.concatenate(cols).astype(np.int32), np.concatenate(y).astype(np.float32)
    if bad:
        at = int(indptr[7] + (indptr[8] - indptr[7]) // 2)
        assert indptr[8] - indptr[7] >= 2
        cols, y = np.insert(cols, at, n_cols + 3), np.insert(y, at, np.float32(5))
        indptr = indptr.copy()
        indptr[8:] += 1
    return indptr, cols, y, (n_rows + len(lens), n_cols)


def _triplets(indptr, cols, y, shape):
    "(rows, cols, y, shape) of the entries that lie inside the matrix, in CSR order"
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    ok = (cols >= 0) & (cols < shape[1])
    return rows[ok], cols[ok].astype(np.int64), y[ok], shape


@pytest.fixture(scope="module")
def edge(counts, gpu):
    "both orientations of the counts with the edge rows, host arrays and device CSR"
    from lkpy_amd import _device as D

    split = D.spmm_split()
    out = {}
    for name, base in (("users", counts), ("items", sps.csr_array(counts.T))):
        base.sort_indices()
        arrays = _edge_rows(base, split, bad=True)
        lens = np.diff(arrays[0])
        n = base.shape[0]
        assert lens[n:].tolist() == [0, 1, split, split + 1, 600]
        out[name] = dict(arrays=arrays, trip=_triplets(*arrays),
                         csr=D.DeviceCSR.from_arrays(*arrays, gpu), first_edge=n)
    return out


def _e_panels(shape, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(-1.0, 1.5, (shape[0], k)).astype(np.float32),
            rng.normal(-1.0, 1.5, (shape[1], k)).astype(np.float32))


# ---- lk_hpf_expect_log --------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_expect_log(gpu, k):
    from lkpy_amd import _device as D

    n = 97
    grid = np.logspace(-3, 6, n * k)
    rng = np.random.default_rng(k)
    shp = rng.permutation(grid).reshape(n, k).astype(np.float32)
    rte = rng.permutation(grid).reshape(n, k).astype(np.float32)
    got = D.hpf_expect_log(D.to_device_padded(shp, gpu), D.to_device_padded(rte, gpu), k)
    got = got.cpu().numpy()
    assert got.shape == (n, D.padded_dim(k)) and not got[:, k:].any()  # pad columns
    psi, lg = digamma(shp.astype(np.float64)), np.log(rte.astype(np.float64))
    want = psi - lg
    bound = U24 * np.abs(want) + 1e-12 * (np.abs(psi) + np.abs(lg))
    err = np.abs(got[:, :k] - want)
    print(f"expect_log k={k}: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ---- lk_hpf_shape_pass --------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("k", KS)
def test_shape_pass(edge, gpu, k, side):
    from lkpy_amd import _device as D

    e = edge[side]
    rows, cols, y, shape = e["trip"]
    er, ec = _e_panels(shape, k, 40 + k)
    prior = 0.3
    d_er, d_ec = D.to_device_padded(er, gpu), D.to_device_padded(ec, gpu)
    out = D.hpf_shape_pass(e["csr"], d_er, d_ec, k, prior)
    again = D.hpf_shape_pass(e["csr"], d_er, d_ec, k, prior)
    got = out.cpu().numpy()
    assert got.shape == (shape[0], D.padded_dim(k)) and not got[:, k:].any()
    assert np.array_equal(_bits(got), _bits(again.cpu().numpy()))
    want = R.shape_sums(rows, cols, y, shape[0], er.astype(np.float64), ec.astype(np.float64),
                        prior)
    yard = R.shape_sums(rows, cols, y, shape[0], er, ec, prior, np.float32)
    d32, ddev = _dist(yard, want), _dist(got[:, :k], want)
    print(f"shape pass {side} k={k}: float32 {d32:.3e} device {ddev:.3e} (bound {4 * d32:.3e})")
    assert d32 > 0 and ddev <= 4.0 * d32
    # the row without entries is the prior, to the bit; the sums are the row's counts
    n0 = e["first_edge"]
    assert np.array_equal(_bits(got[n0, :k]), _bits(np.full(k, np.float32(prior))))
    total = np.bincount(rows, weights=y, minlength=shape[0])
    assert np.allclose(got[:, :k].sum(1, dtype=np.float64) - k * prior, total, rtol=1e-5,
                       atol=1e-4)


def test_shape_pass_row_is_a_function_of_the_row_alone(edge, gpu):
    "every edge row (and a plain one) alone in a one-row matrix has the bits it has in the whole"
    from lkpy_amd import _device as D

    e = edge["users"]
    indptr, cols, y, shape = e["arrays"]
    for k in (16, 20, 100):
        er, ec = _e_panels(shape, k, 7)
        d_ec = D.to_device_padded(ec, gpu)
        whole = D.hpf_shape_pass(e["csr"], D.to_device_padded(er, gpu), d_ec, k, 0.3).cpu().numpy()
        for r in [7, 12] + list(range(e["first_edge"], shape[0])):
            lo, hi = indptr[r], indptr[r + 1]
            # the row stands third of five in another matrix, with other offsets before it
            ptr = np.array([0, 3, 3, 3 + hi - lo, 3 + hi - lo, 5 + hi - lo], dtype=np.int64)
            c1 = np.concatenate([cols[:3], cols[lo:hi], cols[:2]])
            y1 = np.concatenate([y[:3], y[lo:hi], y[:2]])
            csr1 = D.DeviceCSR.from_arrays(ptr, c1, y1, (5, shape[1]), gpu)
            er1 = np.zeros((5, k), np.float32)
            er1[2] = er[r]
            one = D.hpf_shape_pass(csr1, D.to_device_padded(er1, gpu), d_ec, k, 0.3).cpu().numpy()
            assert np.array_equal(_bits(one[2]), _bits(whole[r])), (k, r)


def test_shape_pass_skips_indices_outside_the_matrix(edge, gpu):
    "the entry with the column n_cols + 3 adds nothing: the bits of the matrix without it"
    from lkpy_amd import _device as D

    e = edge["users"]
    indptr, cols, y, shape = e["arrays"]
    bad = np.flatnonzero(cols >= shape[1])
    assert len(bad) == 1 and indptr[7] < bad[0] < indptr[8] - 1
    ptr2 = indptr.copy()
    ptr2[8:] -= 1
    clean = D.DeviceCSR.from_arrays(ptr2, np.delete(cols, bad), np.delete(y, bad), shape, gpu)
    for k in (3, 64):
        er, ec = _e_panels(shape, k, 9)
        d_er, d_ec = D.to_device_padded(er, gpu), D.to_device_padded(ec, gpu)
        a = D.hpf_shape_pass(e["csr"], d_er, d_ec, k, 0.3).cpu().numpy()
        b = D.hpf_shape_pass(clean, d_er, d_ec, k, 0.3).cpu().numpy()
        assert np.array_equal(_bits(a), _bits(b))
        # a negative index and offsets that describe no entries: nothing, and an empty row
        cols3 = cols.copy()
        cols3[bad] = -1
        ptr3 = indptr.copy()
        ptr3[13] = len(cols) + 50  # rows 12 and 13 lose their extent
        odd = D.DeviceCSR.from_arrays(ptr3, cols3, y, shape, gpu)
        c = D.hpf_shape_pass(odd, d_er, d_ec, k, 0.3).cpu().numpy()
        keep = np.ones(shape[0], bool)
        keep[[12, 13]] = False
        assert np.array_equal(_bits(c[keep]), _bits(a[keep]))
        assert np.array_equal(_bits(c[12, :k]), _bits(np.full(k, np.float32(0.3))))


@pytest.mark.parametrize("k", [3, 64, 100])
def test_shape_pass_spread_beyond_the_exp_range(edge, gpu, k):
    """E rows whose components lie 300 apart: the underflowed components weigh zero, nothing is
    NaN, and the output is the restatement's"""
    from lkpy_amd import _device as D

    e = edge["users"]
    rows, cols, y, shape = e["trip"]
    rng = np.random.default_rng(3)
    lead = np.arange(shape[0]) % k
    er = (-300.0 * ((np.arange(k)[None, :] - lead[:, None]) % k)).astype(np.float32)
    ec = rng.normal(0.0, 0.5, (shape[1], k)).astype(np.float32)
    got = D.hpf_shape_pass(e["csr"], D.to_device_padded(er, gpu), D.to_device_padded(ec, gpu), k,
                           0.3).cpu().numpy()[:, :k]
    assert np.isfinite(got).all()
    want = R.shape_sums(rows, cols, y, shape[0], er.astype(np.float64), ec.astype(np.float64), 0.3)
    yard = R.shape_sums(rows, cols, y, shape[0], er, ec, 0.3, np.float32)
    total = np.bincount(rows, weights=y, minlength=shape[0])
    off = np.arange(k)[None, :] != lead[:, None]
    # all the weight on the leading component, exactly the prior everywhere else
    assert np.array_equal(_bits(got[off]), _bits(np.full(off.sum(), np.float32(0.3))))
    assert np.array_equal(_bits(yard[off]), _bits(got[off]))
    assert _dist(got[~off], want[~off]) <= 4.0 * max(_dist(yard[~off], want[~off]),
                                                     U24 * (0.3 + total.max()))
    assert np.allclose(got[~off], 0.3 + total, rtol=1e-5)


def test_shape_pass_rejects_bad_arguments(edge, gpu):
    from lkpy_amd import _device as D

    e = edge["users"]
    shape = e["arrays"][3]
    er, ec = _e_panels(shape, 16, 1)
    d_er, d_ec = D.to_device_padded(er, gpu), D.to_device_padded(ec, gpu)
    with pytest.raises(ValueError, match="alias"):
        D.hpf_shape_pass(e["csr"], d_er, d_ec, 16, 0.3, out=d_er)
    with pytest.raises(ValueError, match="embedding size"):
        from lkpy_amd import _native

        lib = _native.require_gpu()
        _native.check(lib.lk_hpf_expect_log(D._ptr(d_er), D._ptr(d_er), 4, 300, 304,
                                            D._ptr(d_er), D._stream()), "lk_hpf_expect_log")


# ---- lk_hpf_rates ---------------------------------------------------------------------------------
def _rates_inputs(n, k, seed):
    rng = np.random.default_rng(seed)
    shp = rng.gamma(2.0, 3.0, (n, k)).astype(np.float32)
    hyper = rng.uniform(0.5, 40.0, n).astype(np.float32)
    other = rng.uniform(5.0, 90.0, k).astype(np.float32)
    return shp, hyper, other


def _run_rates(shp, hyper, other, k, shp_hyper, ratio, gpu):
    from lkpy_amd import _device as D

    d_shp = D.to_device_padded(shp, gpu)
    d_hyper = torch.from_numpy(hyper.copy()).to(gpu)
    rte, mean = torch.full_like(d_shp, 7.0), torch.full_like(d_shp, 7.0)
    colsum = torch.full((k,), -1.0, dtype=torch.float32, device=gpu)
    D.hpf_rates(d_shp, k, shp_hyper, ratio, d_hyper, torch.from_numpy(other).to(gpu), rte, mean,
                colsum)
    return rte.cpu().numpy(), mean.cpu().numpy(), d_hyper.cpu().numpy(), colsum.cpu().numpy()


@pytest.mark.parametrize("k", KS)
def test_rates(gpu, k):
    n = 300
    shp, hyper, other = _rates_inputs(n, k, 60 + k)
    shp_hyper, ratio = 0.3 + k * 0.3, 0.3
    rte, mean, new_hyper, colsum = _run_rates(shp, hyper, other, k, shp_hyper, ratio, gpu)
    assert not rte[:, k:].any() and not mean[:, k:].any()
    f64 = np.float64
    w_rte, w_mean, _, _ = R.rates(shp.astype(f64), shp_hyper, ratio, hyper.astype(f64),
                                  other.astype(f64))
    y_rte, y_mean, _, _ = R.rates(shp, shp_hyper, ratio, hyper, other, np.float32)
    for name, got, want, yard in (("rte", rte, w_rte, y_rte), ("mean", mean, w_mean, y_mean)):
        d32, ddev = _dist(yard, want), _dist(got[:, :k], want)
        print(f"rates k={k} {name}: float32 {d32:.3e} device {ddev:.3e}")
        assert d32 > 0 and ddev <= 4.0 * d32
    # the sums are float64 sums of the device's own means, rounded once
    m = mean[:, :k].astype(f64)
    rowsum = np.zeros(n)
    for c in range(k):
        rowsum += m[:, c]  # column order
    assert np.array_equal(_bits(new_hyper), _bits((ratio + rowsum).astype(np.float32)))
    exact = m.sum(axis=0)
    near = exact.astype(np.float32)
    assert (np.abs(colsum.astype(f64) - exact) <= np.spacing(near).astype(f64)).all()


def test_rates_do_not_depend_on_the_grid(gpu):
    "300 rows and 300 + one block of rows whose shape is zero: every output has the same bits"
    from lkpy_amd import _device as D

    k, n, more = 20, 300, D.hpf_rates_block()
    assert more == 256
    shp, hyper, other = _rates_inputs(n, k, 8)
    a = _run_rates(shp, hyper, other, k, 6.3, 0.3, gpu)
    shp2 = np.concatenate([shp, np.zeros((more, k), np.float32)])
    hyper2 = np.concatenate([hyper, np.ones(more, np.float32)])
    b = _run_rates(shp2, hyper2, other, k, 6.3, 0.3, gpu)
    for x, z in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(x), _bits(z[:n]))
    assert np.array_equal(_bits(a[3]), _bits(b[3]))
    assert np.array_equal(_bits(b[2][n:]), _bits(np.full(more, np.float32(0.3))))


# ---- lk_hpf_loglik_rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_loglik_rows(edge, gpu, k):
    from lkpy_amd import _device as D

    e = edge["users"]
    rows, cols, y, shape = e["trip"]
    rng = np.random.default_rng(k)
    theta = (rng.uniform(0.5, 1.5, (shape[0], k)) / k).astype(np.float32)
    beta = (rng.uniform(0.5, 1.5, (shape[1], k)) / k).astype(np.float32)
    got = D.hpf_loglik_rows(e["csr"], D.to_device_padded(theta, gpu),
                            D.to_device_padded(beta, gpu), k).cpu().numpy()
    want = R.loglik_rows(rows, cols, y, shape[0], theta, beta)
    assert got.dtype == np.float64 and got[e["first_edge"]] == 0.0
    err = np.abs(got - want)
    print(f"loglik rows k={k}: largest relative error {float((err / np.abs(want).clip(1)).max()):.3e}")
    assert (err <= 1e-12 * np.abs(want)).all()


@pytest.mark.parametrize("k", KS)
def test_loglik_rows_shared_by_a_workgroup(gpu, k):
    """rows beyond 1 024 entries are turned into terms by all groups of a workgroup, 256 ... 4 096
    entries per round by k: exactly 1 024 (still one group), 1 025, 4 200 (two rounds at k <= 16,
    17 at k = 256) with an index outside the matrix, a short row after them"""
    from lkpy_amd import _device as D

    rng = np.random.default_rng(100 + k)
    lens = [1024, 1025, 4200, 0, 5]
    n_cols = 150
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = rng.integers(0, n_cols, indptr[-1]).astype(np.int32)
    cols[indptr[2] + 3000] = n_cols  # no column of the matrix
    y = rng.integers(1, 30, indptr[-1]).astype(np.float32)
    shape = (len(lens), n_cols)
    theta = (rng.uniform(0.5, 1.5, (shape[0], k)) / k).astype(np.float32)
    beta = (rng.uniform(0.5, 1.5, (n_cols, k)) / k).astype(np.float32)
    csr = D.DeviceCSR.from_arrays(indptr, cols, y, shape, gpu)
    got = D.hpf_loglik_rows(csr, D.to_device_padded(theta, gpu), D.to_device_padded(beta, gpu),
                            k).cpu().numpy()
    rows, c, v, _ = _triplets(indptr, cols, y, shape)
    assert len(rows) == indptr[-1] - 1
    want = R.loglik_rows(rows, c, v, shape[0], theta, beta)
    assert got[3] == 0.0 and (got[[0, 1, 2, 4]] < 0).all()
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    # in entry order: the float64 terms added one after the other give the same bits or the next
    dot = np.einsum("ec,ec->e", theta[rows].astype(np.float64), beta[c].astype(np.float64))
    seq = np.cumsum((v * np.log(dot))[rows == 2])[-1]
    assert abs(got[2] - seq) <= 1e-13 * abs(seq)


# ---- the iteration ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_matrix(counts):
    "the counts with the edge rows and no index outside the matrix: (arrays, triplets)"
    from lkpy_amd import _device as D

    arrays = _edge_rows(counts, D.spmm_split(), bad=False)
    return arrays, _triplets(*arrays)


def _device_fit(arrays, panels, iters, gpu, **hp):
    from lkpy_amd import _device as D

    st = D.HPFState(D.DeviceCSR.from_arrays(*arrays, gpu), panels, **hp)
    st.iterate(iters)
    return st


@pytest.mark.parametrize("k", [16, 100])
def test_trajectory(fit_matrix, gpu, k):
    arrays, trip = fit_matrix
    shape = arrays[3]
    hp = R.hyper(a=0.4, c_prime=0.2, b_prime=1.5)
    panels = R.start_panels(shape[0], shape[1], k, np.random.default_rng(k), hp)
    s64, s32 = R.init_state(panels, hp), R.init_state(panels, hp, np.float32)
    for _ in range(8):
        s64, s32 = R.iterate(s64, trip, hp), R.iterate(s32, trip, hp, np.float32)
    st = _device_fit(arrays, panels, 8, gpu, **hp)
    theta, beta = st.host_factors()
    assert st.iterations == 8 and theta.shape == (shape[0], k) and beta.shape == (shape[1], k)
    for name, got in (("theta", theta), ("beta", beta)):
        d32, ddev = _dist(s32[name], s64[name]), _dist(got, s64[name])
        print(f"trajectory k={k} {name}: float32 {d32:.3e} device {ddev:.3e} "
              f"(bound {4 * d32:.3e})")
        assert d32 > 0 and ddev <= 4.0 * d32
    ll = st.loglik()
    want = R.loglik(s64, trip, 0.0)
    assert abs(ll - want) <= 1e-5 * abs(want)
    # a second fit from the same state: identical bits
    t2, b2 = _device_fit(arrays, panels, 8, gpu, **hp).host_factors()
    assert np.array_equal(_bits(t2), _bits(theta)) and np.array_equal(_bits(b2), _bits(beta))


# ---- stopping -----------------------------------------------------------------------------------------
# Chosen from the float64 restatement's trajectory on the counts (k = 16, start drawn from
# default_rng(2), verified on the CPU): with check_every = 5 the relative changes 1 - L / L_prev at
# the checks are 3.76e-1, 1.91e-2, 2.50e-1, 1.63e-1, 2.21e-2, 7.50e-3, 4.13e-3, 2.28e-3, 9.70e-4,
# 1.02e-4.  stop_thr = 3e-4 lies a factor 3.2 below the change at the check before the stop
# (9.701e-4, iteration 45) and a factor 2.9 above the change at the stopping check (1.017e-4,
# iteration 50).
STOP_K, STOP_EVERY, STOP_THR, STOP_AT = 16, 5, 3e-4, 50


def _dataset(mat, with_counts=True):
    from lkpy_amd.data import Dataset, Vocabulary

    coo = mat.tocoo()
    users = Vocabulary(np.arange(1000, 1000 + mat.shape[0]), "user")
    items = Vocabulary(np.arange(5000, 5000 + mat.shape[1]), "item")
    return Dataset(users, items, coo.row, coo.col, {"count": coo.data} if with_counts else {})


def test_stopping(counts, gpu):
    from lkpy_amd.hpf import HPFScorer

    ds = _dataset(counts)
    panels = R.start_panels(N_USERS, N_ITEMS, STOP_K, np.random.default_rng(2))
    _, n_iter, lls = R.fit(counts, panels, maxiter=100, check_every=STOP_EVERY, stop_thr=STOP_THR)
    changes = [1.0 - b / a for a, b in zip(lls[:-1], lls[1:])]
    print("stopping: the restatement's changes", [f"{c:.3e}" for c in changes])
    assert n_iter == STOP_AT and changes[-1] * 1.5 < STOP_THR < changes[-2] / 1.5
    sc = HPFScorer(features=STOP_K, check_every=STOP_EVERY, stop_thr=STOP_THR)
    sc._start_state = panels
    sc.train(ds)
    assert sc.n_iter_ == n_iter and len(sc.loglik_) == len(lls)
    rel = np.abs(np.array(sc.loglik_) / np.array(lls) - 1.0)
    print(f"stopping: largest relative distance of the log-likelihoods {rel.max():.3e}")
    assert (rel <= 1e-6).all()
    every = HPFScorer(features=STOP_K, stop_crit="maxiter", maxiter=STOP_AT + 3)
    every._start_state = panels
    every.train(ds)
    assert every.n_iter_ == STOP_AT + 3 and every.loglik_ == []
    assert np.isfinite(every.user_features).all()


def test_seeds(counts, gpu):
    "random_seed fixes the start whatever the options' generator; without it the options decide"
    from lkpy_amd.hpf import HPFScorer
    from lkpy_amd.training import TrainingOptions

    ds = _dataset(counts)

    def fit(opts, **cfg):
        sc = HPFScorer(features=8, maxiter=2, stop_crit="maxiter", **cfg)
        sc.train(ds, opts)
        return sc.user_features

    a, b = fit(TrainingOptions(rng=1), random_seed=5), fit(TrainingOptions(rng=2), random_seed=5)
    assert np.array_equal(_bits(a), _bits(b))
    c, d, e = (fit(TrainingOptions(rng=s)) for s in (1, 1, 2))
    assert np.array_equal(_bits(c), _bits(d)) and not np.array_equal(_bits(c), _bits(e))
    # the start is the stated one: the draws of default_rng(5) in the stated order
    sc = HPFScorer(features=8, maxiter=2, stop_crit="maxiter")
    sc._start_state = R.start_panels(N_USERS, N_ITEMS, 8, np.random.default_rng(5))
    sc.train(ds)
    assert np.array_equal(_bits(sc.user_features), _bits(a))


# ---- the component on ml-latest-small ------------------------------------------------------------------
UNKNOWN_USER = -777


@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module", params=["counts", "indicator"])
def trained(request, ml, gpu):
    "ratings + 0.5 as counts, and no value column at all (the reference's two tests)"
    from lkpy_amd.data import Dataset
    from lkpy_amd.hpf import HPFScorer
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    if request.param == "counts":
        ds = Dataset(ml.users, ml.items, ml._rows, ml._cols,
                     {"count": np.asarray(ml._attrs["rating"], np.float32) + np.float32(0.5)})
    else:
        ds = Dataset(ml.users, ml.items, ml._rows, ml._cols, {})
    pipe = topn_pipeline(HPFScorer(features=20, maxiter=20))
    pipe.train(ds, TrainingOptions(rng=13))
    return ds, pipe


def test_component(trained, gpu):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.hpf import HPFScorer
    from lkpy_amd.training import TrainingOptions

    ds, pipe = trained
    sc = pipe.node("scorer").component
    assert isinstance(sc, HPFScorer) and sc.is_trained()
    P, Q = sc.user_features, sc.item_features
    assert P.shape == (ds.user_count, 20) and Q.shape == (ds.item_count, 20)
    assert P.dtype == np.float32 and Q.dtype == np.float32
    assert np.isfinite(P).all() and np.isfinite(Q).all() and (P > 0).all() and (Q > 0).all()
    assert sc.user_embeddings is P and sc.item_embeddings is Q
    assert sc.user_bias is None and sc.item_bias is None
    assert 1 <= sc.n_iter_ <= 20 and len(sc.loglik_) >= 2 and sc.loglik_[1] > sc.loglik_[0]

    # __call__: one row of the dense scores, NaN for unknown items and unknown users
    items = ItemList(item_ids=np.concatenate([ds.items.ids()[:300], [-5, -6]]))
    uid = ds.users.ids()[17]
    got = sc(uid, items).scores()
    assert got.dtype == np.float32 and np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()
    want = Q[:300].astype(np.float64) @ P[17].astype(np.float64)
    assert (np.abs(got[:-2] - want) <= 1e-5 * np.abs(want)).all()
    assert np.isnan(sc(UNKNOWN_USER, items).scores()).all()
    assert np.isnan(sc(None, items).scores()).all()
    lists = [ItemList(item_ids=np.concatenate([ds.items.ids()[5 * i:5 * i + 20 + i], [-5]]))
             for i in range(6)]
    users = [ds.users.ids()[3 * i].item() for i in range(5)] + [UNKNOWN_USER]
    for u, il, one in zip(users, lists, sc.score_batch(users, lists)):
        assert np.array_equal(_bits(sc(u, il).scores()), _bits(one.scores()))
        assert np.isnan(one.scores()).all() == (u == UNKNOWN_USER)
    panel, valid, _ = sc.dense_scores_batch(pipe.node("history-lookup").component.batch(
        np.array([uid, UNKNOWN_USER])))
    assert valid.tolist() == [True, False]
    assert np.array_equal(_bits(panel[0].cpu().numpy()),
                          _bits(sc(uid, ItemList.from_vocabulary(ds.items)).scores()))

    # the pipeline: 50 items for 50 users; batch.recommend == pipe.run, items and score bits
    for u in ds.users.ids()[:50]:
        assert len(pipe.run("recommender", query=u.item(), n=50)) == 50
    uids = [int(u) for u in ds.users.ids()[::2][:299]] + [UNKNOWN_USER]
    recs = batch.recommend(pipe, uids, 20)
    assert len(recs) == 300
    for u in uids:
        one = pipe.run("recommender", query=u, n=20)
        il = recs.lookup(u)
        assert np.array_equal(il.ids(), one.ids())
        if len(one):
            assert np.array_equal(_bits(il.scores()), _bits(one.scores()))
    assert len(recs.lookup(UNKNOWN_USER)) == 0
    lookup = pipe.node("history-lookup").component
    idx, val = sc.recommend_batch(lookup.batch(np.array([uid, UNKNOWN_USER])), 10)
    assert (idx[0] >= 0).all() and (idx[1] == -1).all() and np.isnan(val[1]).all()

    # a pickle round trip keeps the factors bit for bit and carries no device state
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__
    assert np.array_equal(_bits(sc2.user_features), _bits(P))
    assert np.array_equal(_bits(sc2.item_features), _bits(Q))
    assert np.array_equal(_bits(sc2(uid, items).scores()[:-2]), _bits(got[:-2]))

    # retrain=False skips
    sc.train(ds, TrainingOptions(retrain=False, rng=99))
    assert sc.item_features is Q and sc.user_features is P


@pytest.mark.parametrize("bad", [0.0, -2.0])
def test_train_rejects_counts_that_are_not_positive(ml, gpu, bad):
    from lkpy_amd.data import Dataset
    from lkpy_amd.hpf import HPFScorer

    vals = np.asarray(ml._attrs["rating"], np.float32).copy()
    vals[1234] = bad
    ds = Dataset(ml.users, ml.items, ml._rows, ml._cols, {"count": vals})
    sc = HPFScorer(features=8)
    with pytest.raises(ValueError, match="positive"):
        sc.train(ds)
    assert not sc.is_trained()


def test_pipeline_file(ml, gpu):
    from lkpy_amd.hpf import HPFScorer
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.training import TrainingOptions

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "hpf.toml")
    sc = pipe.node("scorer").component
    assert isinstance(sc, HPFScorer) and sc.config.embedding_size == 20
    assert sc.config.option("maxiter") == 20
    pipe.train(ml, TrainingOptions(rng=3))
    recs = pipe.run("recommender", query=ml.users.ids()[5].item(), n=10)
    assert len(recs) == 10 and np.isfinite(recs.scores()).all()
