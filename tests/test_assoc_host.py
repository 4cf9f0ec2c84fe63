"""
Association rules without a GPU: the configuration, the reference's ``pipelines/biased-lift.toml``,
the NumPy restatement (``tests/assoc_restatement.py``) against hand-computed probability, lift and
damped lift on a toy matrix, the power of the kernel test's order check on its own input, and the
C ABI's declarations.
"""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import assoc_restatement as R

GOLDEN = Path(__file__).parent / "golden"
f32, f64 = np.float32, np.float64


def test_config():
    from pydantic import ValidationError

    from lkpy_amd.knn import AssociationConfig, AssociationScorer

    cfg = AssociationConfig()
    assert cfg.method == "probability" and cfg.damping == 0.0 and cfg.max_nbrs is None
    with pytest.raises(ValidationError):
        AssociationConfig(nnbrs=3)  # extra="forbid"
    with pytest.raises(ValidationError):
        AssociationConfig(damping=-0.5)
    with pytest.raises(ValidationError):
        AssociationConfig(method="jaccard")
    with pytest.raises(ValidationError):
        AssociationConfig(max_nbrs=0)
    scorer = AssociationScorer(method="lift", damping=10.5, max_nbrs=1)
    assert scorer.config.damping == 10.5 and not scorer.is_trained()
    assert scorer.accepts_history_batch


def test_biased_lift_toml_loads():
    from lkpy_amd.knn import AssociationScorer
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "biased-lift.toml")
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, AssociationScorer) and not scorer.is_trained()
    assert scorer.config.method == "lift" and scorer.config.damping == 20
    assert scorer.config.max_nbrs is None


def _toy():
    "4 users x 5 items: u0 {0,1,2}, u1 {0,1}, u2 {0,3}, u3 {1,2}; nobody rated item 4"
    users = [0, 0, 0, 1, 1, 2, 2, 3, 3]
    items = [0, 1, 2, 0, 1, 0, 3, 1, 2]
    return sps.csr_array((np.ones(9, np.float32), (users, items)), shape=(4, 5))


# pair -> number of users holding both (both orders); every other pair never co-occurs
TOY_PAIRS = {(0, 1): 2, (0, 2): 1, (0, 3): 1, (1, 2): 2}
TOY_COUNTS = [3, 3, 2, 1, 0]


def test_restatement_on_the_toy_matrix():
    cooc, counts, n_groups = R.cooc_counts(_toy())
    assert counts.tolist() == TOY_COUNTS and counts.dtype == np.int32 and n_groups == 4
    want_c = np.zeros((5, 5), np.int64)
    for (a, b), c in TOY_PAIRS.items():
        want_c[a, b] = want_c[b, a] = c
    assert np.array_equal(cooc.toarray(), want_c) and cooc.nnz == 8  # no diagonal, no zeros
    for method, damping in (("probability", 0.0), ("lift", 0.0), ("lift", 20.0),
                            ("probability", 0.5)):
        s = R.train(cooc, counts, n_groups, method, damping)
        assert s.dtype == np.float32 and s.nnz == 8 and s.indptr[4] == s.indptr[5]  # empty row
        assert (1, 3) not in zip(*s.nonzero())
        for (a, b), c in TOY_PAIRS.items():
            for r, t in ((a, b), (b, a)):
                v = f32(f64(f32(c)) / (f64(TOY_COUNTS[r]) + damping))  # by hand, step by step
                if method == "lift":
                    v = f32(v * f32(4))
                    v = f32(f64(v) / (f64(TOY_COUNTS[t]) + damping))
                assert s[r, t].view(np.uint32) == v.view(np.uint32), (method, damping, r, t)
    # the plain values one expects: P[1|0] = 2/3, lift(0, 3) = (1/3) * 4 / 1, damped 4 * 2 / 23^2
    p = R.train(cooc, counts, n_groups)
    assert p[0, 1] == f32(2 / 3) and p[3, 0] == 1.0 and p[2, 0] == 0.5
    lift = R.train(cooc, counts, n_groups, "lift")
    assert abs(float(lift[0, 3]) - 4 / 3) < 1e-6
    damped = R.train(cooc, counts, n_groups, "lift", 20.0)
    assert abs(float(damped[0, 1]) - 8 / 529) < 1e-8

    # scoring: mean over the reference items in order, absent cells 0.0 (not NaN)
    got = R.scores(p, [1, 0])
    assert got[3] == f32(f64(f32(0.0) + p[0, 3]) / 2.0) and got[4] == 0.0
    assert R.scores(p, [1])[3] == 0.0  # items 1 and 3 never co-occur
    assert not np.isnan(R.scores(p, [4])).any() and (R.scores(p, [4]) == 0).all()  # empty row
    assert np.isnan(R.scores(p, [])).all() and np.isnan(R.scores(p, [-1, -1])).all()
    assert np.array_equal(R.scores(p, [0, -1, 0]), R.scores(p, [0, 0]))  # unknown dropped
    assert np.array_equal(R.scores(p, [1, 0], max_nbrs=1),
                          np.maximum(p[[1], :].toarray()[0], p[[0], :].toarray()[0]))
    with pytest.raises(NotImplementedError):
        R.scores(p, [0], max_nbrs=5)
    # top-n: own items struck, a heap over the rest
    idx, sc = R.topn(got, [1, 0], 2, lambda s, n: np.argsort(-np.nan_to_num(s, nan=-1))[:n])
    assert idx.tolist() == [2, 3] and np.array_equal(sc, got[[2, 3]])


@pytest.mark.parametrize("n_items", [65, 8193])
def test_order_of_reference_items_shows_in_the_mean(n_items):
    """The kernel test compares bits: on its own synthetic input a reversed reference list must
    change the bits of a mean cell (else the comparison could not see a reordered sum) and of no
    max cell."""
    s, queries = R.kernel_case(n_items)
    assert len(queries) == R.N_QUERIES and np.diff(s.indptr)[:3].tolist() == [n_items, 0, 1]
    assert s.data.min() < 1e-5 and s.data.max() > 1e2
    q = queries[4]
    assert len(q) == 300 and (np.diff(s.indptr)[q] > 0).all()
    shared = n_items // 2
    assert all(shared in s.indices[s.indptr[r]:s.indptr[r + 1]] for r in np.unique(q))
    mean_f, mean_r = R.scores(s, q), R.scores(s, q[::-1])
    changed = int((mean_f.view(np.uint32) != mean_r.view(np.uint32)).sum())
    assert changed >= 1, "the mean does not depend on the order on this input"
    max_f, max_r = R.scores(s, q, 1), R.scores(s, q[::-1], 1)
    assert np.array_equal(max_f.view(np.uint32), max_r.view(np.uint32))
    desc = queries[5]
    known = desc[desc >= 0]
    assert (np.diff(known) < 0).all() and (desc < 0).sum() == 1


def test_header_declares_and_native_binds_the_entry_points():
    from lkpy_amd import _native

    names = _native.declared_symbols()
    lib = _native.load(build_if_missing=True)
    sigs = _native._declare(lib)
    for name in ("lk_assoc_scale", "lk_assoc_score_batch", "lk_assoc_window"):
        assert name in names and name in sigs and hasattr(lib, name)
    text = _native.HEADER_PATH.read_text()
    for macro in ("LK_ASSOC_PROBABILITY 0", "LK_ASSOC_LIFT 1", "LK_ASSOC_MEAN 0", "LK_ASSOC_MAX 1"):
        assert f"#define {macro}" in text
    assert _native.ASSOC_METHODS == {"probability": 0, "lift": 1}
    assert _native.ASSOC_REDUCTIONS == {"mean": 0, "max": 1}
    w = lib.lk_assoc_window()
    assert w >= 64 and w % 64 == 0 and 4 * w <= 64 * 1024  # static LDS of one workgroup
