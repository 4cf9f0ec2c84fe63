"""
``lk_spd_inverse_blocked`` (csrc/spd_blocked.hip) on the device: one block, a ragged last block,
three and more blocks (the sums of its steps (b) and (c) then span blocks), a leading dimension
above n, the ml-latest-small Gramian.  The yardstick is the one of tests/test_ease_host.py: the
distance from the float64 inverse may be at most 4 x that of LAPACK's float32 ``spotrf`` /
``spotri`` on the same matrix, both computed here.  A matrix whose second block is indefinite
gives flag 2 and a finite result, and ``EASEScorer.train`` raises.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import ease_restatement as er

pytestmark = pytest.mark.gpu


def _rand_binary(n_users, n_items, density, seed):
    m = sps.random(n_users, n_items, density=density, random_state=np.random.default_rng(seed),
                   format="csr", dtype=np.float32)
    m.data[:] = 1.0
    return sps.csr_array(m)


def _invert(gpu, g: np.ndarray, pad: int = 0):
    "The device inverse of ``g`` held in a matrix ``pad`` columns wider: (inverse, flag, padding)."
    import torch

    from lkpy_amd import _device as D

    n = g.shape[0]
    whole = torch.full((n, n + pad), -7.0, dtype=torch.float32, device=gpu)
    whole[:, :n] = torch.from_numpy(g).to(gpu)
    _, flag = D.spd_inverse_blocked(whole[:, :n])
    out = whole.cpu().numpy()
    return out[:, :n], int(flag.item()), out[:, n:]


def _held_to_lapack(inv, g, what):
    ref = np.linalg.inv(g.astype(np.float64))
    d_dev = er.rel_dist(inv, ref)
    # (n = 1: LAPACK's result may be exact; one unit roundoff is then the yardstick, as on the host)
    d_lapack = max(er.rel_dist(er.lapack_inverse_f32(g), ref), 2.0 ** -24)
    print(f"{what}: device {d_dev:.3e}, LAPACK f32 {d_lapack:.3e}, ratio {d_dev / d_lapack:.2f}")
    assert d_dev <= 4 * d_lapack, (d_dev, d_lapack)


@pytest.mark.parametrize("n,pad", [(1, 0), (127, 0), (128, 0), (129, 0), (300, 0), (300, 5),
                                   (515, 0)])
def test_random_gramian(gpu, n, pad):
    g = er.ease_gramian(_rand_binary(2 * n + 10, n, 0.1, seed=n), 1.0)
    inv, flag, padding = _invert(gpu, g, pad)
    assert flag == 0
    assert np.array_equal(inv, inv.T)  # exactly symmetric
    assert np.all(padding == -7.0)
    _held_to_lapack(inv, g, f"n = {n}, ld = n + {pad}")


def test_ml_small_top_1500(gpu, ml_small):
    g = er.ease_gramian(er.top_items_matrix(ml_small, 1500), 1.0)
    inv, flag, _ = _invert(gpu, g)
    assert flag == 0
    assert np.array_equal(inv, inv.T)
    _held_to_lapack(inv, g, "ml-small top 1500, reg = 1")


def test_two_runs_same_bits(gpu):
    g = er.ease_gramian(_rand_binary(700, 300, 0.1, seed=3), 1.0)
    a = _invert(gpu, g)[0]
    b = _invert(gpu, g)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_indefinite_second_block(gpu):
    g = er.indefinite_second_block()
    inv, flag, _ = _invert(gpu, g)
    assert flag == 2 == er.spd_inverse_blocked(g)[1]
    assert np.isfinite(inv).all()
    g[3, 3] = -1.0  # the first failing block is the one reported
    assert _invert(gpu, g)[1] == 1


def test_refuses_what_it_does_not_serve(gpu):
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    lib = _native.require_gpu()
    most = D.spd_inverse_blocked_max_n()
    assert lib.lk_spd_inverse_blocked_workspace_bytes(most + 1) == 0
    x = torch.eye(4, dtype=torch.float32, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(16, dtype=torch.uint8, device=gpu)
    rc = lib.lk_spd_inverse_blocked(D._ptr(x), most + 1, most + 1, D._ptr(ws), 16, D._ptr(flag),
                                    D._stream())
    assert rc == _native.LK_E_INVALID
    rc = lib.lk_spd_inverse_blocked(D._ptr(x), 4, 4, D._ptr(ws), 16, D._ptr(flag), D._stream())
    assert rc == _native.LK_E_INVALID  # workspace too small


def test_ease_train_raises_on_indefinite_gramian(gpu, monkeypatch):
    "``LK_EASE_SOLVER=native``: a non-zero flag is the reference's RuntimeError (ease.py:202-203)."
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.data import Dataset
    from lkpy_amd.knn import EASEScorer
    from lkpy_amd.training import TrainingOptions

    ui = _rand_binary(400, 200, 0.06, seed=11).tocoo()
    ds = Dataset.from_arrays(ui.row + 1000, ui.col + 10, np.ones(ui.nnz, np.float32))
    bad = torch.from_numpy(er.indefinite_second_block(ds.item_count)).to(gpu)
    monkeypatch.setattr(D, "ease_gram", lambda *a, **k: bad.clone())
    with pytest.raises(RuntimeError, match="is not positive-definite"):
        EASEScorer().train(ds, TrainingOptions(environment={"LK_EASE_SOLVER": "native"}))
