"""
The blocked Cholesky inverse of EASE's training, host side: the NumPy restatement of
``lk_spd_inverse_blocked`` (tests/ease_restatement.py -- float32 GEMMs, float64 diagonal blocks)
against the float64 inverse, with LAPACK's float32 ``spotrf`` / ``spotri`` -- the path of
``oracle.ease_train`` -- as the yardstick: the restatement may stand at most 4 x as far from
float64 as LAPACK's float32 does on the same matrix (the project's margin for "as good as the
float32 reference").  No device.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import ease_restatement as er


def _rand_binary(n_users, n_items, density, seed=42):
    m = sps.random(n_users, n_items, density=density, random_state=np.random.default_rng(seed),
                   format="csr", dtype=np.float32)
    m.data[:] = 1.0
    return sps.csr_array(m)


@pytest.fixture(scope="module")
def cases(ml_small):
    "name -> (binary matrix, reg): the ml-small top-1500 items and a random 400 x 300 matrix"
    return {"ml1500": (er.top_items_matrix(ml_small, 1500), 1.0),
            "rand300": (_rand_binary(400, 300, 0.06), 1.0)}


@pytest.mark.parametrize("name", ["ml1500", "rand300"])
def test_restatement_as_close_to_float64_as_lapack(cases, oracle, name):
    ui, reg = cases[name]
    g = er.ease_gramian(ui, reg)
    ref = np.linalg.inv(g.astype(np.float64))
    inv, flag = er.spd_inverse_blocked(g)
    assert flag == 0
    assert np.array_equal(inv, inv.T)
    d_blocked = er.rel_dist(inv, ref)
    d_lapack = er.rel_dist(er.lapack_inverse_f32(g), ref)
    print(f"{name}: inverse: blocked {d_blocked:.3e}, LAPACK f32 {d_lapack:.3e}, "
          f"ratio {d_blocked / d_lapack:.2f}")
    assert d_blocked <= 4 * d_lapack
    # ... and the weights, against the oracle's own training
    w_ref = er.ease_weights(ref)
    w_blocked = er.rel_dist(er.ease_weights(inv), w_ref)
    w_lapack = er.rel_dist(oracle.ease_train(ui, reg), w_ref)
    print(f"{name}: weights: blocked {w_blocked:.3e}, oracle {w_lapack:.3e}, "
          f"ratio {w_blocked / w_lapack:.2f}")
    assert w_blocked <= 4 * w_lapack


@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_restatement_block_edges(n):
    "One block, a ragged last block, three blocks: still an inverse, exactly symmetric."
    g = er.ease_gramian(_rand_binary(2 * n + 10, n, 0.1, seed=n), 1.0)
    ref = np.linalg.inv(g.astype(np.float64))
    inv, flag = er.spd_inverse_blocked(g)
    assert flag == 0 and np.array_equal(inv, inv.T)
    assert er.rel_dist(inv, ref) <= 4 * max(er.rel_dist(er.lapack_inverse_f32(g), ref), 2.0 ** -24)


def test_indefinite_second_block_flags_and_stays_finite():
    g = er.indefinite_second_block()
    inv, flag = er.spd_inverse_blocked(g)
    assert flag == 2
    assert np.isfinite(inv).all()
    # the first block alone is fine; an indefinite first block is block 1
    assert er.spd_inverse_blocked(g[:er.NB, :er.NB])[1] == 0
    g[3, 3] = -1.0
    assert er.spd_inverse_blocked(g)[1] == 1
