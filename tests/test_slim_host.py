"""
SLIM / fsSLIM without a GPU: the NumPy restatement of ``compute_column``
(``tests/slim_restatement.py``; src/accel/slim/mod.rs:147-300) against a closed form and its
invariants, the configuration, the host-side errors of ``train_slim`` and the reference's
``pipelines/slim.toml``.
"""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

from slim_restatement import csr_pair, slim_column

GOLDEN = Path(__file__).parent / "golden"


def _two_items(n):
    "items 0 and 1 rated by the same n users (of n + 2) and by nobody else; item 2 by nobody"
    rows = np.repeat(np.arange(n), 2)
    cols = np.tile([0, 1], n)
    return sps.csr_array((np.ones(2 * n, np.float32), (rows, cols)), shape=(n + 2, 3))


def test_restatement_closed_form():
    """Two items with the same 3 users: the column of one holds (n - l1) / (n + l2) = 0.5 on the
    other -- every float32 step exact --, round 2 recomputes it (diff = 0) and the loop stops."""
    m = csr_pair(_two_items(3))
    for item, other in ((0, 1), (1, 0)):
        info = {}
        idx, val = slim_column(*m, item, 1.0, 1.0, 100, None, info)
        assert idx.tolist() == [other] and val.dtype == np.float32
        assert val.view(np.uint32).tolist() == [np.float32(0.5).view(np.uint32)]
        assert info["rounds"] == 2 and info["active"] == 1 and not info["cut"]
    # l1 = 4 > n: the threshold is not reached, the row is empty, one round
    info = {}
    idx, val = slim_column(*m, 0, 4.0, 1.0, 100, None, info)
    assert len(idx) == 0 and len(val) == 0 and info["rounds"] == 1
    # an item nobody rated: no active item, an empty row
    idx, val = slim_column(*m, 2, 1.0, 1.0, 100, None)
    assert len(idx) == 0 and len(val) == 0


def test_restatement_invariants_on_ml_small(ml_small):
    rmat = sps.csr_array(ml_small["rmat"])
    m = csr_pair(rmat)
    ui_ptr, ui_idx, iu_ptr, iu_idx = m
    n_of = np.diff(iu_ptr)
    rng = np.random.default_rng(5)
    rated = np.flatnonzero(n_of > 0)
    light = rated[n_of[rated] <= 20]
    cols = np.concatenate([rng.choice(light, 6, replace=False), [np.argsort(-n_of)[40]]])
    unrated = int(np.flatnonzero(n_of == 0)[0])
    for k in (None, 25):
        for c in cols:
            info = {}
            idx, val = slim_column(*m, int(c), 1.0, 1.0, 100, k, info)
            assert np.all(val >= np.float32(1e-12)) and c not in idx
            assert np.all(np.diff(idx) > 0)
            users = iu_idx[iu_ptr[c]:iu_ptr[c + 1]]
            co = np.unique(np.concatenate([ui_idx[ui_ptr[u]:ui_ptr[u + 1]] for u in users]))
            assert np.isin(idx, co).all()  # every index is a co-rated item
            if k is not None:
                assert len(idx) <= k and info["kept"] == min(k, info["active"])
        idx, val = slim_column(*m, unrated, 1.0, 1.0, 100, k)
        assert len(idx) == 0 and len(val) == 0


@pytest.mark.parametrize("field", ["l1_reg", "l2_reg", "max_iters", "max_nbrs"])
@pytest.mark.parametrize("bad", [0, -1])
def test_config_validation(field, bad):
    from pydantic import ValidationError

    from lkpy_amd.knn import SLIMConfig, SLIMScorer

    cfg = SLIMConfig()
    assert (cfg.l1_reg, cfg.l2_reg, cfg.max_iters, cfg.max_nbrs) == (1.0, 1.0, 100, None)
    with pytest.raises(ValidationError):
        SLIMConfig(**{field: bad})
    with pytest.raises(ValidationError):
        SLIMScorer(**{field: bad})
    assert SLIMScorer(max_nbrs=500).config.max_nbrs == 500
    assert not SLIMScorer().is_trained()


def test_train_slim_errors_need_no_gpu():
    from lkpy_amd._accel import slim
    from lkpy_amd.matrix import SparseRowArray

    rng = np.random.default_rng(3)
    ui = sps.random_array((30, 12), density=0.2, format="csr", dtype=np.float32, rng=rng)
    sra = lambda m, **kw: SparseRowArray.from_scipy(sps.csr_array(m), values=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="user count mismatch"):
        slim.train_slim(sra(ui), sra(ui[:29].T), 1.0, 1.0, 10, None)
    with pytest.raises(ValueError, match="item count mismatch"):
        slim.train_slim(sra(ui), sra(ui[:, :11].T), 1.0, 1.0, 10, None)
    other = ui.copy().tolil()
    r, c = next((r, c) for r in range(30) for c in range(12) if ui[r, c] == 0)
    other[r, c] = 1.0
    with pytest.raises(ValueError, match="rating count mismatch"):
        slim.train_slim(sra(ui), sra(other.tocsr().T), 1.0, 1.0, 10, None)
    # consistent inputs (32- and 64-bit offsets) give a task without touching a device
    task = slim.train_slim(sra(ui), sra(ui.T, large=True), 1.0, 1.0, 10, 5)
    assert task.current_progress() == (0, 12)
    # a row naming a column twice is refused: the kernels walk a row's entries side by side
    dup_ui = SparseRowArray.from_arrays(np.array([0, 2], np.int32), np.array([1, 1], np.int32),
                                        shape=(1, 3))
    dup_iu = SparseRowArray.from_arrays(np.array([0, 0, 2, 2], np.int32),
                                        np.array([0, 0], np.int32), shape=(3, 1))
    with pytest.raises(ValueError, match="twice"):
        slim.train_slim(dup_ui, dup_iu, 1.0, 1.0, 10, None)


def test_slim_toml_loads():
    from lkpy_amd.knn import SLIMScorer
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "slim.toml")
    scorer = pipe.node("scorer").component
    assert isinstance(scorer, SLIMScorer) and scorer.config.max_nbrs == 500
    assert scorer.config.l1_reg == 1.0 and scorer.config.max_iters == 100
    assert pipe.node("history-lookup").component is not None


def test_new_entry_points_are_declared_and_documented():
    "the ABI / INTEGRATION tests of tests/test_native_abi.py cover these; named here as well"
    from lkpy_amd import _native

    names = {"lk_slim_train_workspace_bytes", "lk_slim_train_count", "lk_slim_train_fill",
             "lk_slim_score_batch", "lk_take_scores"}
    assert names <= set(_native.declared_symbols())
    text = (Path(__file__).parent.parent / "INTEGRATION.md").read_text()
    assert all(n in text for n in names)
