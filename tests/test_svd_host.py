"""
The SVD scorer's host side: its configuration, and the NumPy restatement of the device trainer
(``tests/svd_restatement.py``) held to scikit-learn's ``TruncatedSVD`` through
``tests/golden/svd_ref.npz`` (made by ``tests/golden/make_svd_fixtures.py``).  No GPU.
"""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import svd_restatement as R

GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "svd_ref.npz")


@pytest.fixture(scope="module")
def model():
    "(global bias, item biases, user biases, residual CSR) of ml-latest-small at damping 5"
    from lkpy_amd.data import load_movielens_npz

    ds = load_movielens_npz(GOLDEN / "ml_small.npz")
    return R.bias_residuals(ds._rows, ds._cols, ds._attrs["rating"],
                            (ds.user_count, ds.item_count), 5.0)


@pytest.fixture(scope="module")
def fits(gold, model):
    "the float64 restatement from the stored start panel, k = 8 and 64"
    return {k: R.randomized_svd(model[3], k, int(gold["n_iter"]),
                                gold["omega"][:, :k + R.OVERSAMPLES], np.float64)
            for k in (8, 64)}


def test_config():
    from pydantic import ValidationError

    from lkpy_amd.sklearn.svd import BiasedSVDConfig, BiasedSVDScorer

    cfg = BiasedSVDConfig()
    assert (cfg.embedding_size, cfg.damping, cfg.algorithm, cfg.n_iter) == (64, 5, "randomized", 5)
    assert BiasedSVDConfig(features=12).embedding_size == 12
    assert BiasedSVDConfig(embedding_size=7).embedding_size == 7
    assert BiasedSVDConfig(algorithm="arpack").algorithm == "arpack"  # validates; train refuses
    with pytest.raises(ValidationError):
        BiasedSVDConfig(algorithm="lanczos")
    sc = BiasedSVDScorer(features=8, n_iter=2)
    assert sc.config.embedding_size == 8 and sc.config.n_iter == 2 and not sc.is_trained()


def test_class_path_resolves():
    from lkpy_amd.pipeline import Pipeline, import_path_string
    from lkpy_amd.sklearn.svd import BiasedSVDScorer

    assert import_path_string("lenskit.sklearn.svd.BiasedSVDScorer") is BiasedSVDScorer
    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "biased-svd.toml")
    assert isinstance(pipe.node("scorer").component, BiasedSVDScorer)


def test_residuals_are_the_bias_models(model):
    "the restatement's residuals = BiasModel.learn + transform_matrix of the package"
    from lkpy_amd.basic import BiasModel
    from lkpy_amd.data import load_movielens_npz

    ds = load_movielens_npz(GOLDEN / "ml_small.npz")
    bias = BiasModel.learn(ds, 5)
    g, ib, ub, resid = model
    assert bias.global_bias == g
    assert np.array_equal(bias.item_biases, ib) and np.array_equal(bias.user_biases, ub)
    mat = bias.transform_matrix(
        ds.interaction_matrix(format="scipy", layout="coo", field="rating")).tocsr()
    mat.sort_indices()
    assert np.array_equal(mat.indptr, resid.indptr) and np.array_equal(mat.indices, resid.indices)
    assert np.array_equal(mat.data.astype(np.float32), resid.data)
    assert resid.shape == (671, 9125)


@pytest.mark.parametrize("k", [8, 64])
def test_restatement_matches_sklearn(gold, fits, k):
    s, comp, xt = fits[k]
    want_s = gold[f"sv_{k}"]
    assert s.shape == (k,) and comp.shape == (k, 9125) and xt.shape == (671, k)
    rel = np.abs(s - want_s).max() / want_s.max()
    got_c = comp if k == 8 else comp[:, gold["comp_cols"]]
    dc = np.abs(got_c - gold[f"comp_{k}"]).max()
    dx = np.abs(xt[gold["xt_users"]] - gold[f"xt_{k}"]).max()
    print(f"k={k}: singular values {rel:.1e} relative, components {dc:.1e}, X_t {dx:.1e}")
    assert rel <= 1e-9
    assert dc <= 1e-6  # (stored as float32)
    assert dx <= 1e-5  # (stored as float32; entries up to ~10)


@pytest.mark.parametrize("k", [8, 64])
def test_restatement_scores(gold, model, fits, k):
    "the scorer's arithmetic on the restatement's factors = the reference formula on sklearn's"
    g, ib, ub, _ = model
    _, comp, xt = fits[k]
    for r, (u, items) in enumerate(zip(gold["score_users"], gold["score_items"])):
        got = R.score(xt[u], comp, items, g, ib, ub[u], np.float64)
        # the reference adds the three biases in float32 before the float64 sum
        assert np.abs(got - gold[f"scores_{k}"][r]).max() <= 1e-6, (k, r)


def test_float32_restatement_distance(gold, model, fits):
    "what the device tests use as their yardstick is of the size the issue measured (~1e-5)"
    s64, comp64, xt64 = fits[8]
    s32, comp32, xt32 = R.randomized_svd(model[3], 8, 5, gold["omega"][:, :18], np.float32)
    assert s32.dtype == np.float64 and comp32.dtype == np.float32 and xt32.dtype == np.float32
    ds = np.abs(s32 - s64).max()
    dr = np.abs(xt32.astype(np.float64) @ comp32 - xt64 @ comp64).max()
    print(f"float32 restatement, k=8: singular values {ds:.1e}, reconstruction {dr:.1e}")
    assert 0 < ds < 1e-3 and 0 < dr < 1e-3


def test_svd_flip_sign_rule():
    comp = np.array([[0.1, -0.9, 0.5], [0.7, 0.2, -0.3], [-0.4, 0.4, 0.1], [0.0, 0.0, 0.0]])
    got = R.svd_flip_v(comp)
    assert np.array_equal(got[0], -comp[0])  # largest magnitude -0.9: flipped
    assert np.array_equal(got[1], comp[1])   # largest magnitude +0.7: kept
    assert np.array_equal(got[2], -comp[2])  # a tie in magnitude: the first entry decides
    assert np.array_equal(got[3], comp[3])   # a zero row stays
    from sklearn.utils.extmath import svd_flip

    rng = np.random.default_rng(0)
    v = rng.normal(size=(5, 40))
    _, want = svd_flip(rng.normal(size=(30, 5)), v.copy(), u_based_decision=False)
    assert np.array_equal(R.svd_flip_v(v), want)


def test_transpose_rule():
    "the restatement operates on the transpose exactly when there are fewer rows than columns"
    assert R.operates_on_transpose((30, 40)) and not R.operates_on_transpose((40, 30))
    assert not R.operates_on_transpose((40, 40))
    rng = np.random.default_rng(1)
    a = sps.random_array((30, 40), density=0.5, rng=rng, dtype=np.float64).tocsr()
    k = 4
    # the start panel has min(shape) rows either way; a panel of the other size is refused
    for mat in (a, sps.csr_array(a.T)):
        omega = rng.normal(size=(30, k + R.OVERSAMPLES))
        s, comp, xt = R.randomized_svd(mat, k, 2, omega)
        assert comp.shape == (k, mat.shape[1]) and xt.shape == (mat.shape[0], k)
        want = np.linalg.svd(mat.toarray(), compute_uv=False)[:k]
        assert np.abs(s - want).max() <= 0.05 * want[0]
        with pytest.raises(AssertionError):
            R.randomized_svd(mat, k, 2, rng.normal(size=(40, k + R.OVERSAMPLES)))
    # the two orientations from one panel: the same singular values, the factors swapped
    omega = rng.normal(size=(30, k + R.OVERSAMPLES))
    s1, c1, x1 = R.randomized_svd(a, k, 3, omega)
    s2, c2, x2 = R.randomized_svd(sps.csr_array(a.T), k, 3, omega)
    assert np.abs(s1 - s2).max() <= 1e-12 * s1[0]
    assert np.abs(np.abs(x1 / s1) - np.abs(c2.T)).max() <= 1e-10
    with pytest.raises(ValueError):
        R.randomized_svd(a, 21, 2, rng.normal(size=(30, 31)))
