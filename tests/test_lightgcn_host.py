"""
LightGCN, host side (no GPU): configuration, the pipeline file, the construction of the graph,
the restatement's own consistency (Horner form against layer sum, autograd against the operator
applied to the pair gradient) and the C ABI's declarations.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import lightgcn_restatement as R

GOLDEN = Path(__file__).parent / "golden"


# ---- configuration ----------------------------------------------------------------------
def test_config_defaults():
    from lkpy_amd.graphs.lightgcn import LightGCNConfig

    c = LightGCNConfig()
    assert (c.embedding_size, c.layer_count, c.layer_blend, c.batch_size) == (16, 2, None, 4096)
    assert (c.learning_rate, c.epochs, c.regularization, c.loss) == (0.01, 10, 0.01, "pairwise")
    assert c.blend_weights() == [1.0 / 3.0] * 3
    assert LightGCNConfig(layer_count=3, layer_blend=0.5).blend_weights() == [0.5] * 4
    assert LightGCNConfig(embedding_size_exp=5).embedding_size == 32
    assert LightGCNConfig(regularization=None).regularization is None
    assert LightGCNConfig(loss="logistic").loss == "logistic"


def test_config_validators():
    from lkpy_amd.graphs.lightgcn import LightGCNConfig, LightGCNScorer

    with pytest.raises(ValueError, match="exceeds the device kernels' limit"):
        LightGCNConfig(embedding_size=257)
    with pytest.raises(ValueError, match="exceeds the device kernels' limit"):
        LightGCNConfig(embedding_size_exp=9)
    assert LightGCNConfig(embedding_size_exp=8).embedding_size == 256
    with pytest.raises(ValueError, match="layer_blend has length 3, expected 2"):
        LightGCNConfig(layer_blend=[0.2, 0.3, 0.5])
    for bad in (dict(loss="warp"), dict(layer_count=0), dict(layer_blend=-1.0),
                dict(regularization=0.0), dict(epochs=0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            LightGCNConfig(**bad)
    # a list of the reference's length validates; the trainer says why it cannot run it
    sc = LightGCNScorer(layer_blend=[0.5, 0.5])
    assert sc.config.layer_blend == [0.5, 0.5]
    with pytest.raises(NotImplementedError, match="layer_blend"):
        sc.create_trainer(None, None)
    assert not sc.is_trained()


def test_pipeline_file_names_the_scorer():
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "lightgcn.toml")
    sc = pipe.node("scorer").component
    assert isinstance(sc, LightGCNScorer)
    assert (sc.config.embedding_size, sc.config.layer_count, sc.config.loss) == (16, 2, "pairwise")


# ---- the graph ----------------------------------------------------------------------------
def test_graph_of_a_hand_written_matrix():
    """3 users x 4 items, user 1 and item 2 empty:
        u0: i0 i1 i3      u1: -      u2: i1 i3
    nodes: items 0..3, users 4..6"""
    from lkpy_amd.graphs.lightgcn import graph_adjacency, initial_table

    indptr, cols = [0, 3, 3, 5], [0, 1, 3, 1, 3]
    m_ptr, m_cols, d = graph_adjacency(indptr, cols, 3, 4)
    assert m_ptr.dtype == np.int64 and m_cols.dtype == np.int32 and d.dtype == np.float32
    assert m_ptr.tolist() == [0, 1, 3, 3, 5, 8, 8, 10]
    assert m_cols.tolist() == [4, 4, 6, 4, 6, 0, 1, 3, 1, 3]
    deg = np.array([1, 2, 0, 2, 3, 0, 2])
    want = np.zeros(7)
    want[deg > 0] = deg[deg > 0] ** -0.5
    assert np.array_equal(d, want.astype(np.float32)) and d[2] == 0 and d[5] == 0
    dense = R.dense_operator(m_ptr, m_cols, np.ones(7))
    assert np.array_equal(dense, dense.T) and dense.sum() == 10  # symmetric, 2 nnz entries
    assert np.array_equal(dense[4:, :4], [[1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 0, 1]])
    assert not dense[:4, :4].any() and not dense[4:, 4:].any()
    # a transpose handed in gives the same graph
    again = graph_adjacency(indptr, cols, 3, 4, transpose=([0, 1, 3, 3, 5], [0, 0, 2, 0, 2]))
    assert all(np.array_equal(a, b) for a, b in zip(again, (m_ptr, m_cols, d)))
    # initialisation: item rows drawn first, then user rows; isolated nodes zeroed
    tab = initial_table(3, 4, 5, torch.Generator().manual_seed(3), degrees=deg)
    gen = torch.Generator().manual_seed(3)
    items = torch.empty((4, 5)).normal_(0.0, 0.1, generator=gen).numpy()
    users = torch.empty((3, 5)).normal_(0.0, 0.1, generator=gen).numpy()
    assert tab.shape == (7, 5) and tab.dtype == np.float32
    assert not tab[2].any() and not tab[5].any()
    keep = deg > 0
    assert np.array_equal(tab[keep], np.concatenate([items, users])[keep])


# ---- the restatement's own consistency ------------------------------------------------------
def _random_graph(rng, n_users=30, n_items=50, k=7):
    from lkpy_amd.graphs.lightgcn import graph_adjacency

    lens = rng.integers(0, 12, n_users)
    lens[3] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(n_items - 2, m, replace=False)) for m in lens])
    m_ptr, m_cols, d = graph_adjacency(indptr, cols.astype(np.int32), n_users, n_items)
    x = rng.normal(0.0, 0.1, (n_users + n_items, k))
    return m_ptr, m_cols, d, x, n_items


@pytest.mark.parametrize("alphas", [[0.5, 0.5], [0.25] * 4, [0.7, 0.2, 0.4]])
def test_horner_form_is_the_layer_sum(alphas):
    m_ptr, m_cols, d, x, _ = _random_graph(np.random.default_rng(1))
    mhat = R.dense_operator(m_ptr, m_cols, d)
    a, b = R.blend_layer_sum(mhat, x, alphas), R.blend_horner(mhat, x, alphas)
    assert np.abs(a).max() > 1e-3
    assert np.abs(a - b).max() <= 1e-12
    # ... and the Horner steps written with propagate_f64, as the device runs them
    t = x
    b_coef = alphas[-1]
    for j in range(len(alphas) - 2, -1, -1):
        t, _ = R.propagate_f64(m_ptr, m_cols, d, alphas[j], x, b_coef, t)
        b_coef = 1.0
    assert np.abs(t - a).max() <= 1e-12
    # the Torch module computes the same embeddings, sparse and dense
    for dense in (False, True):
        tr = R.TorchTrainer(x, m_ptr, m_cols, d, alphas, dtype=torch.float64, dense=dense)
        assert np.abs(tr.final_embeddings() - a).max() <= 1e-12


@pytest.mark.parametrize("loss", ["pairwise", "logistic"])
def test_autograd_gradient_is_the_operator_on_the_pair_gradient(loss):
    rng = np.random.default_rng(2)
    m_ptr, m_cols, d, x, n_items = _random_graph(rng)
    alphas = [0.4, 0.3, 0.3]
    B = 64
    users = rng.integers(0, 30, B) + n_items
    users[:10] = users[0]
    pos, neg = rng.integers(0, n_items, B), rng.integers(0, n_items, B)
    neg[5] = pos[6]
    tr = R.TorchTrainer(x * 10, m_ptr, m_cols, d, alphas, loss=loss, dtype=torch.float64)
    auto = tr.table_gradient(users, pos, neg)
    _, g = tr.pair_gradient(tr.final_embeddings(), users, pos, neg)
    touched = np.unique(np.concatenate([users, pos, neg]))
    assert not np.delete(g, touched, axis=0).any()  # non-zero only on the batch's rows
    mhat = R.dense_operator(m_ptr, m_cols, d)
    want = R.blend_layer_sum(mhat, g, alphas)
    assert np.abs(auto).max() > 1e-4
    assert np.abs(auto - want).max() <= 1e-12
    assert np.abs(auto - R.blend_horner(mhat, g, alphas)).max() <= 1e-12


def test_losses_are_as_stated():
    sp = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64)
    sn = torch.tensor([0.1, 0.4, -0.5], dtype=torch.float64)
    sig = torch.sigmoid
    assert abs(float(R.batch_loss("pairwise", sp, sn)) - float((-torch.log(sig(sp - sn))).mean())) < 1e-15
    want = (-torch.log(sig(sp))).sum() + (-torch.log(sig(-sn))).sum()
    assert abs(float(R.batch_loss("logistic", sp, sn)) - float(want) / 6) < 1e-15


# ---- C ABI ---------------------------------------------------------------------------------
def test_abi_declares_the_kernels():
    from lkpy_amd import _native

    names = _native.declared_symbols()
    for name in ("lk_lgcn_propagate", "lk_lgcn_pair_grad", "lk_lgcn_pair_grad_workspace_bytes",
                 "lk_adamw_dense"):
        assert name in names
