"""CPU: the host side of hierarchical Poisson factorization -- ``HPFConfig`` (defaults, aliases,
rejected extras, non-positive hyper-parameters), the NumPy / SciPy restatement
(tests/hpf_restatement.py) against a brute-force dense evaluation of one iteration, the
restatement's log-likelihood over a fit, and the declared entries."""
import numpy as np
import pytest
import scipy.sparse as sps
from scipy.special import digamma

import hpf_restatement as R


# ---- configuration -----------------------------------------------------------------------------
def test_config_defaults_and_aliases():
    from lkpy_amd.hpf import HPFConfig, HPFScorer

    cfg = HPFConfig()
    assert cfg.count_attribute == "count" and cfg.embedding_size == 64
    assert cfg.hyper() == dict(a=0.3, a_prime=0.3, b_prime=1.0, c=0.3, c_prime=0.3, d_prime=1.0)
    assert (cfg.option("maxiter"), cfg.option("stop_crit"), cfg.option("check_every"),
            cfg.option("stop_thr"), cfg.option("random_seed")) == (100, "train-llk", 10, 1e-3, None)
    assert HPFConfig(features=20).embedding_size == 20
    assert HPFConfig(embedding_size=7).embedding_size == 7
    s = HPFScorer(features=12, a=0.5, maxiter=30, stop_crit="maxiter", random_seed=4,
                  count_attribute=None)
    assert s.config.embedding_size == 12 and s.config.count_attribute is None
    assert s.config.hyper()["a"] == 0.5 and s.config.option("maxiter") == 30
    assert s.config.option("stop_crit") == "maxiter" and s.config.option("random_seed") == 4
    assert not s.is_trained()
    assert HPFScorer({"features": 5}).config.embedding_size == 5
    assert HPFScorer._start_state is None


@pytest.mark.parametrize("extra", ["reindex", "ncores", "k", "users_per_batch"])
def test_config_rejects_other_extras(extra):
    from lkpy_amd.hpf import HPFScorer

    with pytest.raises(ValueError) as err:
        HPFScorer(**{extra: 1})
    assert extra in str(err.value) and "hpfrec is not behind" in str(err.value)


@pytest.mark.parametrize("name", ["a", "a_prime", "b_prime", "c", "c_prime", "d_prime"])
@pytest.mark.parametrize("value", [0.0, -0.3])
def test_config_rejects_non_positive_hyper_parameters(name, value):
    from lkpy_amd.hpf import HPFScorer

    with pytest.raises(ValueError, match=name):
        HPFScorer(**{name: value})


def test_config_rejects_bad_sizes_and_criteria():
    from lkpy_amd.hpf import HPFScorer

    for bad in (dict(features=0), dict(features=257), dict(stop_crit="val-llk"),
                dict(maxiter=0), dict(check_every=0)):
        with pytest.raises(ValueError):
            HPFScorer(**bad)


def test_declared_symbols_name_the_entries():
    from lkpy_amd import _native

    names = _native.declared_symbols()
    for want in ("lk_hpf_expect_log", "lk_hpf_shape_pass", "lk_hpf_rates", "lk_hpf_loglik_rows",
                 "lk_hpf_rates_workspace_bytes"):
        assert want in names


# ---- the restatement against a dense evaluation ---------------------------------------------
def _small(seed=3, n_users=12, n_items=9, k=4):
    rng = np.random.default_rng(seed)
    dense = rng.poisson(0.8, (n_users, n_items)).astype(np.float64)
    dense[5] = 0  # a user without entries
    dense[:, 2] = 0  # an item without entries
    panels = R.start_panels(n_users, n_items, k, rng)
    return dense, panels, k


def _dense_iteration(dense, st, hp, k):
    "one iteration by explicit loops over every (user, item, component)"
    n_users, n_items = dense.shape
    e_u = digamma(st["g_shp"]) - np.log(st["g_rte"])
    e_i = digamma(st["l_shp"]) - np.log(st["l_rte"])
    g_shp = np.full((n_users, k), hp["a"])
    l_shp = np.full((n_items, k), hp["c"])
    for u in range(n_users):
        for i in range(n_items):
            if dense[u, i] > 0:
                w = np.exp(e_u[u] + e_i[i])
                phi = dense[u, i] * w / w.sum()
                g_shp[u] += phi
                l_shp[i] += phi
    g_rte = ((hp["a_prime"] + k * hp["a"]) / st["k_rte"])[:, None] + st["beta"].sum(0)[None, :]
    theta = g_shp / g_rte
    k_rte = hp["a_prime"] / hp["b_prime"] + theta.sum(1)
    l_rte = ((hp["c_prime"] + k * hp["c"]) / st["t_rte"])[:, None] + theta.sum(0)[None, :]
    beta = l_shp / l_rte
    t_rte = hp["c_prime"] / hp["d_prime"] + beta.sum(1)
    return dict(g_shp=g_shp, g_rte=g_rte, l_shp=l_shp, l_rte=l_rte, theta=theta, beta=beta,
                k_rte=k_rte, t_rte=t_rte, T=theta.sum(0), S=beta.sum(0))


def test_restatement_start():
    dense, panels, k = _small()
    for p, base in zip(panels, (0.3, 1.0, 0.3, 1.0)):
        assert p.dtype == np.float32 and (p >= np.float32(base)).all()
        assert (p < np.float32(base) + np.float32(0.0100001)).all()
    st = R.init_state(panels)
    assert np.allclose(st["k_rte"], 0.3 + (st["g_shp"] / st["g_rte"]).sum(1), rtol=1e-14)
    assert np.allclose(st["t_rte"], 0.3 + st["beta"].sum(1), rtol=1e-14)
    assert np.allclose(st["S"], st["beta"].sum(0), rtol=1e-14)


def test_restatement_iteration_matches_dense_evaluation():
    dense, panels, k = _small()
    hp = R.hyper(a=0.4, c_prime=0.2, b_prime=1.5)
    st = R.init_state(panels, hp)
    mat = sps.csr_array(dense)
    for _ in range(2):  # the second iteration starts from a state that is no start
        want = _dense_iteration(dense, st, hp, k)
        st = R.iterate(st, mat, hp)
        for name, w in want.items():
            assert np.abs(st[name] - w).max() <= 1e-12 * np.abs(w).max(), name
    # rows and columns without entries stay at the prior shape
    assert (st["g_shp"][5] == hp["a"]).all() and (st["l_shp"][2] == hp["c"]).all()


def test_restatement_loglik_matches_dense_evaluation_and_rises():
    from math import lgamma

    dense, panels, k = _small()
    mat = sps.csr_array(dense)
    st0 = R.init_state(panels)

    def dense_ll(st):
        lam = st["theta"] @ st["beta"].T
        on = dense > 0
        return float((dense[on] * np.log(lam[on])).sum() - lam.sum()
                     - sum(lgamma(v + 1.0) for v in dense[on]))

    assert abs(R.loglik(st0, mat) - dense_ll(st0)) <= 1e-12 * abs(dense_ll(st0))
    st = st0
    for _ in range(20):
        st = R.iterate(st, mat)
    assert abs(R.loglik(st, mat) - dense_ll(st)) <= 1e-12 * abs(dense_ll(st))
    assert R.loglik(st, mat) > R.loglik(st0, mat)


def test_restatement_fit_stops_and_runs_out():
    dense, panels, k = _small()
    mat = sps.csr_array(dense)
    st, n_iter, lls = R.fit(mat, panels, maxiter=40, check_every=5, stop_thr=1e-3)
    assert n_iter % 5 == 0 and len(lls) == n_iter // 5 + 1
    if n_iter < 40:
        assert 1.0 - lls[-1] / lls[-2] < 1e-3
    assert all(1.0 - b / a >= 1e-3 for a, b in zip(lls[:-2], lls[1:-1]))
    st, n_iter, lls = R.fit(mat, panels, maxiter=13, stop_crit="maxiter")
    assert n_iter == 13 and lls == []


def test_float32_restatement_is_close_but_not_equal():
    dense, panels, k = _small()
    mat = sps.csr_array(dense)
    s64, s32 = R.init_state(panels), R.init_state(panels, dtype=np.float32)
    for _ in range(3):
        s64, s32 = R.iterate(s64, mat), R.iterate(s32, mat, dtype=np.float32)
    assert s32["theta"].dtype == np.float32 and s32["k_rte"].dtype == np.float32
    d = np.abs(s32["theta"] - s64["theta"]).max()
    assert 0 < d < 1e-5 * np.abs(s64["theta"]).max()


def test_count_matrix_sums_duplicates_and_checks_values():
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.hpf import count_matrix

    users, items = Vocabulary(np.arange(3)), Vocabulary(np.arange(4))
    rows, cols = np.array([0, 0, 1, 2, 0]), np.array([1, 1, 3, 0, 2])
    ds = Dataset(users, items, rows, cols, {"count": np.array([2.0, 3.0, 1.0, 4.0, 1.0])})
    mat = count_matrix(ds, "count")
    assert mat.nnz == 4 and mat[0, 1] == 5.0
    assert count_matrix(ds, None).toarray()[0, 1] == 2.0  # indicator counts, summed as well
    no_count = Dataset(users, items, rows, cols, {})
    assert count_matrix(no_count, "count").toarray()[0, 1] == 2.0
    for bad in (0.0, -1.0, np.nan, np.inf):
        ds = Dataset(users, items, rows, cols, {"count": np.array([2.0, 3.0, bad, 4.0, 1.0])})
        with pytest.raises(ValueError, match="positive"):
            count_matrix(ds, "count")
