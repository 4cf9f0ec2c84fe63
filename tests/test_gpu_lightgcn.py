"""
LightGCN on the device (csrc/lightgcn.hip, lkpy_amd/graphs/lightgcn.py) against the NumPy / Torch
restatement of ``tests/lightgcn_restatement.py``.

The propagate kernel is held to a derived bound: a chain of ``len`` fused multiply-adds rounds
each product term at most ``len`` times (cut into segments and added in segment order: fewer),
the row's scale ``b d_r``, its product with the sum and the fused ``a x`` term round three more
times, so every entry is within (len + 3) 2^-24 (|a x| + |b| d_r sum d_c |t_c|) of the float64
product.

Everything that goes through transcendental functions and an optimiser is held to the project's
criterion (``tests/test_gpu_flexmf.py``): the distance of the device from the FLOAT64 Torch
restatement is at most 4 x the distance of the FLOAT32 Torch restatement from it, computed in the
same test from the same inputs.
"""
import json
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

import lightgcn_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ml():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


# ---- the graphs -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_graph():
    """40 users x 700 items: user 0 has 600 items (three chain segments), user 1 has 257 (two),
    user 2 exactly 256 (one), user 3 exactly one, user 4 none; items 690.. have no user."""
    from lkpy_amd.graphs.lightgcn import graph_adjacency

    rng = np.random.default_rng(5)
    n_users, n_items = 40, 700
    lens = rng.integers(2, 40, n_users)
    lens[:5] = [600, 257, 256, 1, 0]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(690, m, replace=False)) for m in lens]).astype(np.int32)
    m_ptr, m_cols, d = graph_adjacency(indptr, cols, n_users, n_items)
    deg = np.diff(m_ptr)
    assert deg[n_items:n_items + 5].tolist() == [600, 257, 256, 1, 0]
    assert (deg[690:700] == 0).all() and (deg[:n_items] <= 256).all()
    return dict(n_users=n_users, n_items=n_items, indptr=indptr, cols=cols, m_ptr=m_ptr,
                m_cols=m_cols, d=d, deg=deg)


@pytest.fixture(scope="module")
def ml_graph(ml):
    from lkpy_amd.graphs.lightgcn import graph_adjacency

    m_ptr, m_cols, d = graph_adjacency(ml._indptr, ml._cols, ml.user_count, ml.item_count)
    return dict(n_users=ml.user_count, n_items=ml.item_count, indptr=ml._indptr, cols=ml._cols,
                m_ptr=m_ptr, m_cols=m_cols, d=d, deg=np.diff(m_ptr))


def _dev_graph(g, gpu):
    return (torch.from_numpy(g["m_ptr"]).to(gpu), torch.from_numpy(g["m_cols"]).to(gpu),
            torch.from_numpy(g["d"]).to(gpu))


def test_device_transpose_builds_the_same_graph(ml, ml_graph, gpu):
    from lkpy_amd import _device as D
    from lkpy_amd.graphs.lightgcn import graph_adjacency

    csr = D.DeviceCSR.from_arrays(np.asarray(ml._indptr, np.int64), ml._cols, None,
                                  (ml.user_count, ml.item_count), gpu)
    t = D.csr_transpose(csr, with_values=False)
    got = graph_adjacency(ml._indptr, ml._cols, ml.user_count, ml.item_count,
                          transpose=(t.indptr.cpu().numpy(), t.indices.cpu().numpy()))
    for a, b in zip(got, (ml_graph["m_ptr"], ml_graph["m_cols"], ml_graph["d"])):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- propagate ----------------------------------------------------------------------------------
PROP_K = [1, 3, 16, 20, 64, 256]


def _panels(n, k, seed, gpu):
    from lkpy_amd import _device as D

    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, k)).astype(np.float32)
    t = rng.normal(0.0, 1.0, (n, k)).astype(np.float32)
    return x, t, D.lgcn_panel(x, gpu), D.lgcn_panel(t, gpu)


@pytest.mark.parametrize("k", PROP_K)
@pytest.mark.parametrize("with_x", [True, False])
def test_propagate(small_graph, gpu, k, with_x):
    from lkpy_amd import _device as D

    g = small_graph
    n = len(g["deg"])
    ptr, cols, d = _dev_graph(g, gpu)
    x, t, dx, dt = _panels(n, k, 100 + k, gpu)
    a, b = np.float32(0.7), np.float32(-1.3)
    out = D.lgcn_propagate(ptr, cols, d, a, dx if with_x else None, b, dt, k)
    again = D.lgcn_propagate(ptr, cols, d, a, dx if with_x else None, b, dt, k)
    got = out.cpu().numpy()
    assert got.shape == (n, D.lgcn_ld(k))
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))
    assert not got[:, k:].any()  # pad columns
    want, size = R.propagate_f64(g["m_ptr"], g["m_cols"], g["d"], float(a), x if with_x else None,
                                 float(b), t)
    bound = (g["deg"][:, None] + 3) * U24 * size
    err = np.abs(got[:, :k] - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"propagate k={k} x={with_x}: largest error / bound {worst:.3f}")
    assert (err <= bound).all()
    # a node without entries: a x bit for bit (0 without x)
    alone = g["deg"] == 0
    assert alone[g["n_items"] + 4] and alone[690:700].all() and alone.sum() >= 11
    want_alone = a * x[alone] if with_x else np.zeros_like(x[alone])
    assert np.array_equal(got[alone, :k].view(np.uint32), want_alone.view(np.uint32))
    # the long rows were not left at their a x term
    assert np.abs(got[g["n_items"], :k] - (a * x[g["n_items"]] if with_x else 0)).max() > 1e-3


def test_propagate_row_is_a_function_of_the_row_alone(small_graph, gpu):
    "the 600-entry row alone in a one-row-heavy matrix has the bits it has in the whole graph"
    from lkpy_amd import _device as D

    g = small_graph
    n, k = len(g["deg"]), 20
    ptr, cols, d = _dev_graph(g, gpu)
    _, _, dx, dt = _panels(n, k, 7, gpu)
    whole = D.lgcn_propagate(ptr, cols, d, 0.5, dx, 2.0, dt, k).cpu().numpy()
    for node in (g["n_items"], g["n_items"] + 1, g["n_items"] + 2, g["n_items"] + 7, 3):
        lo, hi = g["m_ptr"][node], g["m_ptr"][node + 1]
        alone_ptr = np.zeros(n + 1, np.int64)
        alone_ptr[node + 1:] = hi - lo
        one = D.lgcn_propagate(torch.from_numpy(alone_ptr).to(gpu),
                               torch.from_numpy(g["m_cols"][lo:hi].copy()).to(gpu), d, 0.5, dx,
                               2.0, dt, k).cpu().numpy()
        assert np.array_equal(one[node].view(np.uint32), whole[node].view(np.uint32)), node


def test_propagate_skips_indices_outside_the_graph(small_graph, gpu):
    from lkpy_amd import _device as D

    g = small_graph
    n, k = len(g["deg"]), 16
    ptr, cols, d = _dev_graph(g, gpu)
    x, t, dx, dt = _panels(n, k, 8, gpu)
    bad = g["m_cols"].copy()
    hit = np.arange(0, len(bad), 7)
    bad[hit[::2]] = -1
    bad[hit[1::2]] = n
    got = D.lgcn_propagate(ptr, torch.from_numpy(bad).to(gpu), d, 1.0, dx, 1.0, dt, k).cpu().numpy()
    keep = np.ones(len(bad), bool)
    keep[hit] = False
    rows = np.repeat(np.arange(n), g["deg"])
    kept_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    want, size = R.propagate_f64(kept_ptr, g["m_cols"][keep], g["d"], 1.0, x, 1.0, t)
    assert (np.abs(got[:, :k] - want) <= (g["deg"][:, None] + 3) * U24 * size).all()


@pytest.mark.parametrize("k", [3, 64])
def test_propagate_is_self_adjoint(small_graph, gpu, k):
    "<M^ t, s> = <t, M^ s> within the per-entry bound summed over the rows"
    from lkpy_amd import _device as D

    g = small_graph
    n = len(g["deg"])
    ptr, cols, d = _dev_graph(g, gpu)
    s, t, ds, dt = _panels(n, k, 9, gpu)
    mt = D.lgcn_propagate(ptr, cols, d, 0.0, None, 1.0, dt, k).cpu().numpy()[:, :k].astype(np.float64)
    ms = D.lgcn_propagate(ptr, cols, d, 0.0, None, 1.0, ds, k).cpu().numpy()[:, :k].astype(np.float64)
    _, size_t = R.propagate_f64(g["m_ptr"], g["m_cols"], g["d"], 0.0, None, 1.0, t)
    _, size_s = R.propagate_f64(g["m_ptr"], g["m_cols"], g["d"], 0.0, None, 1.0, s)
    scale = (g["deg"][:, None] + 3) * U24
    bound = float((scale * size_t * np.abs(s)).sum() + (scale * size_s * np.abs(t)).sum())
    lhs, rhs = float((mt * s).sum()), float((t * ms).sum())
    print(f"adjoint k={k}: {lhs:.9f} vs {rhs:.9f}, |difference| {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs) > 1e-3
    assert abs(lhs - rhs) <= bound


def test_propagate_rejects_bad_arguments(small_graph, gpu):
    from lkpy_amd import _device as D

    g = small_graph
    ptr, cols, d = _dev_graph(g, gpu)
    _, _, dx, dt = _panels(len(g["deg"]), 16, 1, gpu)
    with pytest.raises(ValueError, match="aliases"):
        D.lgcn_propagate(ptr, cols, d, 1.0, dx, 1.0, dt, 16, out=dt)
    with pytest.raises(ValueError, match="leading dimension"):
        D.lgcn_propagate(ptr, cols, d, 1.0, dx, 1.0, dt, 17)
    with pytest.raises(ValueError, match="embedding size"):
        D.lgcn_propagate(ptr, cols, d, 1.0, dx, 1.0, dt, 0)


# ---- pair gradient -------------------------------------------------------------------------------
def _state(g, k, gpu, alphas=(0.5, 0.5), table=None, **kw):
    from lkpy_amd import _device as D

    n = len(g["deg"])
    if table is None:
        table = np.zeros((n, k), np.float32)
    return D.LightGCNState(table, g["m_ptr"], g["m_cols"], g["d"], list(alphas), dev=gpu, **kw)


def _pair_batches(g, rng, last):
    "(users, positives, negatives) as node numbers: the four batch shapes of the issue"
    n_users, n_items = g["n_users"], g["n_items"]

    def draw(B):
        return (rng.integers(0, n_users, B) + n_items, rng.integers(0, n_items, B),
                rng.integers(0, n_items, B))

    one = draw(1)
    u, p, n = draw(64)
    same_user = (np.full(64, u[0]), p, n)
    u, p, n = draw(300)
    n[:50] = p[100:150]  # a negative that is another sample's positive
    n[50] = p[50]        # ... and one that is its own
    crossed = (u, p, n)
    return {"one": one, "same user": same_user, "crossed": crossed, "short last": draw(last)}


@pytest.mark.parametrize("loss", ["pairwise", "logistic"])
@pytest.mark.parametrize("which", ["small", "ml"])
def test_pair_gradient(small_graph, ml_graph, gpu, which, loss):
    """g and the loss of every batch against float64 autograd, each batch by the 4 x criterion on
    its own.  One exception: the loss of the one-sample batch is ONE float32 number, whose
    distance from the float64 value is a rounding error of any size between 0 and half an ulp and
    no yardstick on its own; it is held to 4 x the largest float32 loss distance of the four
    batches instead.  Its g (3 rows of k numbers) is held to its own distance like the others."""
    from lkpy_amd import _device as D

    g = small_graph if which == "small" else ml_graph
    n, k = len(g["deg"]), 20
    rng = np.random.default_rng(11)
    xbar = rng.normal(0.0, 0.5, (n, k)).astype(np.float32)
    st = _state(g, k, gpu, loss=loss)
    d_xbar = D.lgcn_panel(xbar, gpu)
    last = len(g["cols"]) % 8192 if which == "ml" else 37  # the short last batch at B = 8192
    assert 0 < last < 8192
    t64 = R.TorchTrainer(xbar, g["m_ptr"], g["m_cols"], g["d"], [0.5, 0.5], loss=loss,
                         dtype=torch.float64)
    t32 = R.TorchTrainer(xbar, g["m_ptr"], g["m_cols"], g["d"], [0.5, 0.5], loss=loss,
                         dtype=torch.float32)
    figures = {}
    for name, (u, p, ng) in _pair_batches(g, rng, last).items():
        l64, g64 = t64.pair_gradient(xbar, u, p, ng)
        l32, g32 = t32.pair_gradient(xbar, u, p, ng)
        gd, ld = st.pair_grad(d_xbar, u, p, ng)
        gd = gd.cpu().numpy()
        assert not gd[:, k:].any()
        touched = np.unique(np.concatenate([u, p, ng]))
        assert not np.delete(gd, touched, axis=0).any()  # zero everywhere else
        assert np.abs(g64).max() > 0
        figures[name] = (float(np.abs(g32 - g64).max()), float(np.abs(gd[:, :k] - g64).max()),
                         abs(l32 - l64), abs(float(ld.item()) - l64))
        print(f"{which}/{loss}/{name}: gradient float32 {figures[name][0]:.3e} device "
              f"{figures[name][1]:.3e}; loss float32 {figures[name][2]:.3e} device "
              f"{figures[name][3]:.3e}")
    e32_all = max(f[2] for f in figures.values())
    for name, (d32, ddev, e32, edev) in figures.items():
        assert d32 > 0, name
        assert ddev <= 4.0 * d32, (name, ddev, d32)
        if name == "one":
            assert e32_all > 0 and edev <= 4.0 * e32_all, (name, edev, e32_all)
        else:
            assert e32 > 0, name
            assert edev <= 4.0 * e32, (name, edev, e32)


def test_pair_gradient_adds_to_the_loss_sum_and_checks_indices(small_graph, gpu):
    from lkpy_amd import _device as D

    g = small_graph
    n, k = len(g["deg"]), 16
    st = _state(g, k, gpu)
    xbar = D.lgcn_panel(np.random.default_rng(0).normal(0, 0.5, (n, k)).astype(np.float32), gpu)
    u, p, ng = np.array([705, 706]), np.array([1, 2]), np.array([3, 4])
    total = torch.full((1,), 2.0, dtype=torch.float32, device=gpu)
    _, loss = st.pair_grad(xbar, u, p, ng, loss_sum=total)
    assert float(total.item()) == np.float32(2.0) + np.float32(loss.item())
    with pytest.raises(ValueError, match="negatives outside"):
        st.pair_grad(xbar, u, p, np.array([3, n]))
    # unchecked, a sample naming no node takes no part (and nothing is written out of bounds)
    gd, loss = st.pair_grad(xbar, np.array([705, 705]), np.array([1, 1]), np.array([3, -1]),
                            check_indices=False)
    g1, l1 = st.pair_grad(xbar, np.array([705]), np.array([1]), np.array([3]),
                          out=torch.empty_like(xbar))
    # (the mean is over the batch's two samples: half the single sample's values)
    assert np.allclose(2 * gd.cpu().numpy(), g1.cpu().numpy(), rtol=1e-6, atol=0)
    assert abs(2 * float(loss.item()) - float(l1.item())) <= 1e-6


# ---- dense AdamW ---------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.01])
@pytest.mark.parametrize("k", [20, 18])
def test_adamw_dense(gpu, k, reg):
    "three steps on a 50 x 20 panel (k = 18: two pad columns), rows and whole steps of zero gradient"
    from lkpy_amd import _device as D

    rng = np.random.default_rng(13)
    p0 = rng.normal(0.0, 0.1, (50, k)).astype(np.float32)
    grads = [rng.normal(0.0, 1e-3, (50, k)).astype(np.float32) for _ in range(3)]
    grads[0][::3] = 0.0
    grads[1][:] = 0.0
    grads[2][10:20] = 0.0
    w64 = R.adamw_steps(p0, grads, regularization=reg, dtype=torch.float64)
    w32 = R.adamw_steps(p0, grads, regularization=reg, dtype=torch.float32)
    p, m, v = D.lgcn_panel(p0, gpu), None, None
    assert tuple(p.shape) == (50, 20)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(grads, start=1):
        D.adamw_dense(p, m, v, D.lgcn_panel(g, gpu), k, step=step, learning_rate=0.01,
                      weight_decay=reg)
    for name, dev, a32, a64 in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), w32, w64):
        dev = dev.cpu().numpy()
        assert not dev[:, k:].any()  # pad columns stay zero
        d32, ddev = np.abs(a32 - a64).max(), np.abs(dev[:, :k] - a64).max()
        print(f"AdamW k={k} reg={reg} {name}: float32 {d32:.3e} device {ddev:.3e}")
        assert d32 > 0
        assert ddev <= 4.0 * d32
    assert np.abs(w64[0] - p0).max() > 1e-3  # (the steps moved the parameters)


# ---- the trainer's batches -------------------------------------------------------------------------
def test_trainer_batches_are_node_numbers_with_true_negatives(ml, gpu):
    """one batch through ``train_batch``'s inputs: users are user NODES, positives their items,
    and the sampler -- its CSR addressed by node -- still rejects the user's training items"""
    import flexmf_restatement as FR
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.training import TrainingOptions

    n_items = ml.item_count
    tr = LightGCNScorer().create_trainer(ml, TrainingOptions(rng=8))
    perm = np.random.default_rng(1).permutation(len(ml._rows)).astype(np.int32)[:8192]
    # the heaviest user's samples too: a fifth of its uniform draws are redrawn
    heavy = int(np.argmax(np.diff(ml._indptr)))
    perm[:500] = np.arange(ml._indptr[heavy], ml._indptr[heavy] + 500)
    users, pos, neg = (t.cpu().numpy() for t in
                       tr.batch_nodes(torch.from_numpy(perm).to(gpu), 3))
    assert np.array_equal(users, ml._rows[perm] + n_items) and np.array_equal(pos, ml._cols[perm])
    assert neg.shape == (8192,) and neg.min() >= 0 and neg.max() < n_items
    keys = FR.pair_keys(ml._indptr, ml._cols, n_items)
    rows = users - n_items
    share = np.diff(ml._indptr)[rows] / n_items
    false_neg = int(FR.reject(keys, n_items, rows, neg).sum())
    print(f"trainer batch: {false_neg} false negatives of 8192, expected {(share ** 11).sum():.2e}")
    assert false_neg <= 3 + 10 * float((share ** 11).sum())  # the bound of the FlexMF sampler test
    assert len(np.unique(neg)) > 4000  # (uniform over the items, not stuck)
    # without rejection the same batch does hold training items
    from lkpy_amd import _device as D
    raw = D.flexmf_sample_negatives(tr.d_node_indptr, tr.d_cols, n_items, users, 1, "uniform",
                                    tr.sample_key, 3, verify=False).cpu().numpy().reshape(-1)
    assert FR.reject(keys, n_items, rows, raw).sum() > 20


# ---- step parity ---------------------------------------------------------------------------------
def _batches(ds, epochs=2, B=8192, seed=3):
    "the fixed permutation and negatives handed to both sides, as node numbers"
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(epochs):
        perm = rng.permutation(len(ds._rows))
        for s in range(0, len(perm), B):
            sel = perm[s:s + B]
            neg = rng.integers(0, ds.item_count, len(sel)).astype(np.int32)
            out.append((ds._rows[sel].astype(np.int32) + ds.item_count, ds._cols[sel], neg))
    return out


def _init(ml, g, k, seed=1):
    from lkpy_amd.graphs.lightgcn import initial_table

    return initial_table(ml.user_count, ml.item_count, k, torch.Generator().manual_seed(seed),
                         degrees=g["deg"])


def _run_device(g, table, alphas, batches, gpu, **kw):
    st = _state(g, table.shape[1], gpu, alphas=alphas, table=table, **kw)
    losses = [st.step(u, p, n) for u, p, n in batches]
    return st.host_table(), torch.cat(losses).cpu().numpy().astype(np.float64), st


def _run_torch(g, table, alphas, batches, dtype, **kw):
    tr = R.TorchTrainer(table, g["m_ptr"], g["m_cols"], g["d"], alphas, dtype=dtype, **kw)
    losses = [tr.step(u, p, n) for u, p, n in batches]
    return tr.table().astype(np.float64), np.asarray(losses, np.float64)


@pytest.fixture(scope="module")
def step_batches(ml):
    batches = _batches(ml)
    assert len(batches) == 26
    return batches


@pytest.mark.parametrize("blend", [None, 0.5])
@pytest.mark.parametrize("loss", ["pairwise", "logistic"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("k", [16, 64])
def test_step_parity(ml, ml_graph, step_batches, gpu, k, L, loss, blend):
    "26 steps (two epochs of ml-latest-small at B = 8192) from the seeded initialisation"
    alphas = [1.0 / (L + 1) if blend is None else blend] * (L + 1)
    table = _init(ml, ml_graph, k)
    kw = dict(loss=loss, regularization=0.01, learning_rate=0.01)
    f64, l64 = _run_torch(ml_graph, table, alphas, step_batches, torch.float64, **kw)
    f32, l32 = _run_torch(ml_graph, table, alphas, step_batches, torch.float32, **kw)
    dev, ldev, _ = _run_device(ml_graph, table, alphas, step_batches, gpu, **kw)
    d32, ddev = float(np.abs(f32 - f64).max()), float(np.abs(dev - f64).max())
    e32, edev = float(np.abs(l32 - l64).max()), float(np.abs(ldev - l64).max())
    print(f"k={k}/L={L}/{loss}/blend={blend}: tables float32 {d32:.3e} device {ddev:.3e} (bound "
          f"{4 * d32:.3e}); losses float32 {e32:.3e} device {edev:.3e} (bound {4 * e32:.3e})")
    assert np.abs(f64 - table).max() > 1e-2  # (the steps moved the parameters)
    assert d32 > 0 and e32 > 0
    assert ddev <= 4.0 * d32
    assert edev <= 4.0 * e32


def test_steps_are_reproducible(ml, ml_graph, step_batches, gpu):
    table = _init(ml, ml_graph, 64)
    runs = [_run_device(ml_graph, table, [0.25] * 4, step_batches[:13], gpu, loss="pairwise")
            for _ in range(2)]
    (a, la, st), (b, lb, _) = runs
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(la, lb)
    assert not st.X[:, 64:].any() and st.steps == 13
    # rows of isolated nodes that no batch named stay exactly zero
    named = np.unique(np.concatenate([np.concatenate(bt) for bt in step_batches[:13]]))
    quiet = np.setdiff1d(np.flatnonzero(ml_graph["deg"] == 0), named)
    assert not a[quiet].any()


# ---- component ------------------------------------------------------------------------------------
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

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "lightgcn.toml")
    pipe.train(ml_plus, TrainingOptions(rng=13))
    return pipe


def test_component(ml_plus, gpu, trained):
    ml = ml_plus
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList, RecQuery
    from lkpy_amd.graphs.lightgcn import LightGCNScorer

    pipe = trained
    sc = pipe.node("scorer").component
    assert isinstance(sc, LightGCNScorer) and sc.is_trained() and sc.trained_epochs == 10
    P, Q = sc.user_embeddings, sc.item_embeddings
    assert P.shape == (ml.user_count, 16) and Q.shape == (ml.item_count, 16)
    assert P.dtype == np.float32 and np.isfinite(P).all() and np.isfinite(Q).all()
    assert sc.user_bias is None and sc.item_bias is None
    # users without interactions: no gradient, no neighbours -- their propagated rows are zero
    empty = ml.users.numbers(np.asarray(EXTRA_USERS))
    assert (np.diff(ml._indptr)[empty] == 0).all() and not P[empty].any()
    assert P[np.diff(ml._indptr) > 0].any(axis=1).all()

    items = ItemList(item_ids=np.concatenate([ml.items.ids()[:300], [-5, -6]]))
    uid = ml.users.ids()[17]
    got = sc(uid, items).scores()
    assert got.dtype == np.float32
    assert np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()  # unknown items
    want = Q[:300].astype(np.float64) @ P[17].astype(np.float64)
    size = np.abs(Q[:300]).astype(np.float64) @ np.abs(P[17])
    assert (np.abs(got[:-2] - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    assert np.isnan(sc(-12345, items).scores()).all()  # an unknown user
    assert np.isnan(sc(None, items).scores()).all()

    # score_batch = __call__, bit for bit, whatever else the batch holds
    lists = [ItemList(item_ids=np.concatenate([ml.items.ids()[5 * i:5 * i + 20 + i], [-5]]))
             for i in range(12)]
    users = [ml.users.ids()[3 * i].item() for i in range(11)] + [-777]
    for u, il, one in zip(users, lists, sc.score_batch(users, lists)):
        assert np.array_equal(sc(u, il).scores().view(np.uint32), one.scores().view(np.uint32))
        assert np.isnan(one.scores()[-1])
        assert np.isnan(one.scores()).all() == (u == -777)
    assert sc.score_batch([], []) == []

    # recommend_batch = the top n of the per-query scores with the history removed, same bits
    lookup = pipe.node("history-lookup").component
    uids = np.concatenate([ml.users.ids()[[3, 17, 99, 400]], [-777]])
    hb = lookup.batch(uids)
    idx, val = sc.recommend_batch(hb, 10)
    assert idx.shape == (5, 10) and (idx[4] == -1).all() and np.isnan(val[4]).all()
    all_items = ItemList.from_vocabulary(ml.items)
    panel, valid, _hist = sc.dense_scores_batch(hb)
    panel = panel.cpu().numpy()
    assert valid.tolist() == [True] * 4 + [False] and np.isnan(panel[4]).all()
    for r, u in enumerate(uids[:4]):
        s = sc(u, all_items).scores().copy()
        assert np.array_equal(s.view(np.uint32), panel[r].view(np.uint32))
        un = ml.users.number(u)
        s[ml._cols[ml._indptr[un]:ml._indptr[un + 1]]] = -np.inf
        assert np.array_equal(val[r].view(np.uint32), s[idx[r]].view(np.uint32))
        assert np.array_equal(val[r].view(np.uint32), np.sort(s)[::-1][:10].view(np.uint32))
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
    for r, u in enumerate(uids[:4]):
        il = recs.lookup(u)
        assert np.array_equal(il.numbers(vocabulary=ml.items), idx[r])
        assert np.array_equal(il.scores().astype(np.float32).view(np.uint32), val[r].view(np.uint32))

    # a pickle round trip holds no device state and scores with the same bits
    sc2 = pickle.loads(pickle.dumps(sc))
    assert "_dev" not in sc2.__dict__ and "_pending_sync" not in sc2.__dict__
    assert np.array_equal(sc2.item_embeddings, Q)
    assert np.array_equal(sc2(uid, items).scores()[:-2].view(np.uint32), got[:-2].view(np.uint32))


def test_retrain_false_skips(ml_plus, gpu, trained):
    from lkpy_amd.training import TrainingOptions

    sc = trained.node("scorer").component
    before = sc.item_embeddings
    sc.train(ml_plus, TrainingOptions(retrain=False, rng=99))
    assert sc.item_embeddings is before


def test_seeds(ml, gpu):
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.training import TrainingOptions

    def fit(seed):
        sc = LightGCNScorer(epochs=2, loss="logistic")
        sc.train(ml, TrainingOptions(rng=seed))
        return sc

    a, b, c = fit(5), fit(5), fit(6)
    assert np.array_equal(a.user_embeddings.view(np.uint32), b.user_embeddings.view(np.uint32))
    assert np.array_equal(a.item_embeddings.view(np.uint32), b.item_embeddings.view(np.uint32))
    assert not np.array_equal(a.item_embeddings, c.item_embeddings)


def test_trainer_parameters_and_epoch_loss(ml, ml_graph, gpu):
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.training import TrainingOptions

    sc = LightGCNScorer(epochs=1, layer_count=3, layer_blend=0.5)
    tr = sc.create_trainer(ml, TrainingOptions(rng=2))
    want = _init(ml, ml_graph, 16, seed=2)
    p0 = tr.get_parameters()
    assert set(p0) == {"embedding.weight"} and np.array_equal(p0["embedding.weight"], want)
    first = tr.train_epoch()["loss"]
    second = tr.train_epoch()["loss"]
    assert 0.0 < second < first < 1.0  # pairwise loss falls from about log 2
    # the lazily refreshed host arrays are the propagated embeddings of the table
    xbar = R.blend_horner(R.dense_operator(ml_graph["m_ptr"], ml_graph["m_cols"], ml_graph["d"]),
                          tr.get_parameters()["embedding.weight"], [0.5] * 4)
    got = np.concatenate([sc.item_embeddings, sc.user_embeddings])
    assert np.abs(got - xbar).max() <= 1e-5 * max(1.0, np.abs(xbar).max())
    p2 = tr.get_parameters()
    tr.load_parameters(p0)
    assert np.array_equal(tr.get_parameters()["embedding.weight"], want)
    tr.load_parameters(p2)
    assert np.array_equal(np.concatenate([sc.item_embeddings, sc.user_embeddings]), got)


def test_largest_embedding_size(ml, gpu):
    "k = 256, the configuration's limit: one epoch trains, and scoring takes 258 columns"
    from lkpy_amd.data import ItemList
    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.training import TrainingOptions

    sc = LightGCNScorer(embedding_size_exp=8, epochs=1)
    sc.train(ml, TrainingOptions(rng=4))
    P, Q = sc.user_embeddings, sc.item_embeddings
    assert P.shape == (ml.user_count, 256) and Q.shape == (ml.item_count, 256)
    assert np.isfinite(P).all() and np.isfinite(Q).all() and P.any()
    got = sc(ml.users.ids()[5], ItemList(item_ids=ml.items.ids()[:200])).scores()
    want = Q[:200].astype(np.float64) @ P[5]
    size = np.abs(Q[:200]).astype(np.float64) @ np.abs(P[5])
    assert (np.abs(got - want) <= 1e-5 * np.maximum(np.abs(want), size)).all()
    idx, val = sc.recommend_batch([ml.users.ids()[5].item()], 5, exclude_history=False)
    full = sc(ml.users.ids()[5], ItemList.from_vocabulary(ml.items)).scores()
    assert np.array_equal(val[0].view(np.uint32), np.sort(full)[::-1][:5].view(np.uint32))


# ---- quality ------------------------------------------------------------------------------------
QUALITY_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("loss", ["pairwise", "logistic"])
def test_quality(ml, gpu, loss):
    """quick_measure_model NDCG against the Torch restatement trainer's five CPU runs
    (tests/golden/lightgcn_quality.json, the protocol of the FlexMF quality check): three fixed
    device seeds each reach the lowest of the five minus their range, so does their mean, and
    every run is above the sanity floor of 0.01."""
    from dataclasses import replace

    from lkpy_amd.graphs.lightgcn import LightGCNScorer
    from lkpy_amd.metrics import quick_measure_model
    from lkpy_amd.training import TrainingOptions

    gold = json.loads((GOLDEN / "lightgcn_quality.json").read_text())
    ref = np.asarray(gold["ndcg"][loss])
    floor = ref.min() - (ref.max() - ref.min())
    assert floor >= 0.01
    vals = []
    for seed in QUALITY_SEEDS:
        class Seeded(LightGCNScorer):
            def train(self, data, options=TrainingOptions(), _seed=seed):
                super().train(data, replace(options, rng=_seed))

        res = quick_measure_model(Seeded(loss=loss, **gold["config"][loss]), ml,
                                  rng=gold["split_seed"])
        vals.append(float(res.list_summary().loc["NDCG", "mean"]))
    print(f"{loss}: NDCG {[round(v, 4) for v in vals]}, mean {np.mean(vals):.4f}; restatement "
          f"{ref.min():.4f} .. {ref.max():.4f} (mean {ref.mean():.4f}), floor {floor:.4f}")
    assert min(vals) >= floor
    assert np.mean(vals) >= floor
    assert min(vals) > 0.01
