"""CPU: the NumPy restatement of the CG row solve (tests/als_cg_restatement.py) against
``np.linalg.solve`` and the float64 oracle, the conditions the GPU tests of csrc/als_cg.hip
(tests/test_gpu_als_cg.py) rely on -- asserted here so that a change of seed or shape cannot
quietly void them -- and the proof that those tests' bounds tell a wrong kernel from a right one."""
import numpy as np
import pytest

import als_cg_restatement as R

CASES = [(k, neg) for k in R.KS for neg in (False, True)]


def test_seam_matrix_is_what_the_gpu_tests_assume():
    for kp in (64, 128, 256):
        ri, tb = R.resident(kp), R.tail_batch(kp)
        assert (ri, tb) == {64: (64, 16), 128: (32, 16), 256: (16, 8)}[kp]
        mat, other, this = R.seam_matrix(kp, 5, negative=True)
        lens = np.diff(mat.indptr)
        want = R.seam_lengths(kp)
        assert sorted(lens.tolist()) == sorted(want * 2 + [0, 0, 0])
        assert {1, ri, ri + 1, 4 * ri, 4 * ri + 1, 4 * ri + tb, 4 * ri + 9 * tb + 3, 2048,
                2049} <= set(want)
        assert 50 <= mat.shape[0] <= 60 and mat.shape[1] == 2100
        # shuffled: the plan's longest-first order is not the row order
        assert not np.array_equal(np.argsort(-lens, kind="stable"), np.arange(len(lens)))
        for r in range(mat.shape[0]):
            idx = mat.indices[mat.indptr[r]:mat.indptr[r + 1]]
            assert np.all(np.diff(idx) > 0) and (len(idx) == 0 or (idx[0] >= 0 and idx[-1] < 2100))
        v = mat.data
        assert v.dtype == np.float32 and other.dtype == np.float32 and this.dtype == np.float32
        assert 0.07 < np.mean(v == 0) < 0.13 and 0.07 < np.mean(v < 0) < 0.13
        assert v.min() >= -2.0 and v.max() <= 40.0
        pos, _, _ = R.seam_matrix(kp, 5)
        assert pos.data.min() == 0.0 and np.array_equal(pos.indices, mat.indices)
        sd = other.std(axis=0)
        assert 0.04 < sd.min() < 0.06 and 0.18 < sd.max() < 0.22


def test_restatement_conventions():
    c = R.case(33)
    empty = int(np.flatnonzero(c.lens == 0)[0])
    x, it, hist = R.cg_row(c.other[:0], c.mat.data[:0], c.otor, c.this[empty], 1e-3)
    assert not x.any() and it == 0 and hist == []
    # max_iter = 0 means k
    r = int(np.argmax(c.lens))
    s, e = c.mat.indptr[r], c.mat.indptr[r + 1]
    q, v = c.other[c.mat.indices[s:e]], c.mat.data[s:e]
    assert R.cg_row(q, v, c.otor, c.this[r], 0.0, 0)[1] == 33
    assert R.cg_row(q, v, c.otor, c.this[r], 0.0, 5)[1] == 5
    x32, it32, _ = R.cg_row(q, v, c.otor, c.this[r], 1e-3, 0, np.float32)
    assert x32.dtype == np.float32


@pytest.mark.parametrize("k,negative", CASES)
def test_float64_cg_is_the_dense_solve(oracle, k, negative):
    c = R.case(k, negative)
    x, its, frob, _ = R.cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-12, 4 * k)
    assert its.max() < 4 * k
    assert R.row_rel(x, c.x).max() <= 1e-9
    assert not x[c.lens == 0].any() and not its[c.lens == 0].any()
    # the delta is the reference's: an empty row is zeroed but counts 0 (implicit.rs:98-101)
    nz = c.lens > 0
    assert abs(frob - np.linalg.norm((x - c.this)[nz])) <= 1e-12 * frob
    assert c.this[~nz].any() and frob < np.linalg.norm(x - c.this) * (1 - 1e-4)
    this = c.this.copy()
    assert abs(oracle.als_half_epoch(c.mat, this, c.other, c.otor) - frob) <= 1e-4 * frob
    assert R.row_rel(this, c.x).max() <= 1e-4
    # ... and the oracle's float64 half-epoch (its own float64 OtOr)
    o64 = c.other.astype(np.float64)
    xo, _, _, _ = R.cg_half_epoch(c.mat, c.this, c.other, o64.T @ o64 + R.REG * np.eye(k), 1e-12,
                                  4 * k)
    assert R.row_rel(xo, oracle.als_half_epoch_f64(c.mat, c.other, R.REG)).max() <= 1e-9


@pytest.mark.parametrize("k,negative", CASES)
def test_conditions_the_gpu_tests_rely_on(k, negative):
    c = R.case(k, negative)
    # 1. well conditioned: the converged bound stays far below a mispaired value's effect
    assert c.cond.max() <= 200, c.cond.max()
    # 2. the iteration sandwich of tol = 1e-3 is narrow
    lo = R.iteration_totals(k, negative, 1.1e-3)
    hi = R.iteration_totals(k, negative, 1e-3 / 1.1)
    assert lo <= R.iteration_totals(k, negative, 1e-3) <= hi
    assert hi - lo <= 0.05 * hi, (lo, hi)
    # 3. the Jacobi diagonal matters
    plain = R.iteration_totals(k, negative, 1e-3, "nojacobi")
    assert plain >= 1.5 * R.iteration_totals(k, negative, 1e-3), (plain, lo, hi)
    # 4. no row is finished within 3 iterations, so `set_cg(1e-20, m)` runs exactly m
    _, its, _, hists = R.cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-20, 3)
    assert np.array_equal(its, np.where(c.lens > 0, 3, 0))
    assert min(min(h) for h in hists if h) > 1e-6
    print(f"\nk {k} negative {negative}: cond <= {c.cond.max():.1f}, sandwich {lo} .. {hi} "
          f"({(hi - lo) / hi:.1%}), unpreconditioned {plain / lo:.2f} x")


@pytest.mark.parametrize("k,negative", CASES)
def test_float32_restatement_takes_the_float64_iterations(k, negative):
    "at tol = 1e-3 r.r is orders above float32 round-off: float32 NumPy stays inside the sandwich"
    c = R.case(k, negative)
    its32 = int(R.cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-3, 2 * k, np.float32)[1].sum())
    assert (R.iteration_totals(k, negative, 1.1e-3) <= its32
            <= R.iteration_totals(k, negative, 1e-3 / 1.1))


@pytest.mark.parametrize("k,negative", CASES)
@pytest.mark.parametrize("variant", ["shift", "nojacobi"])
def test_fixed_iteration_bound_sees_a_wrong_kernel(k, negative, variant):
    """Each value paired with the next entry of its row, or a lost preconditioner: every row of
    two or more entries then leaves the bound the GPU rows are held to after m iterations."""
    c = R.case(k, negative)
    rows = c.lens >= 2
    for m in (1, 2, 3):
        x64, _, e32 = R.fixed_iterations(k, negative, m)
        bound = R.fixed_bound(e32.max())
        assert bound < 5e-5, bound
        wrong, _, _, _ = R.cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-20, m, variant=variant)
        moved = R.row_rel(wrong, x64)[rows]
        assert moved.min() > 100 * bound, (m, moved.min(), bound)


@pytest.mark.parametrize("k,negative", CASES)
def test_iteration_sandwich_sees_a_lost_preconditioner(k, negative):
    assert (R.iteration_totals(k, negative, 1e-3, "nojacobi")
            > R.iteration_totals(k, negative, 1e-3 / 1.1))


@pytest.mark.parametrize("k", R.KS)
def test_converged_bound_sees_a_mispaired_value(k):
    "the converged answer of the shifted system is outside the bound of every row it changes"
    c = R.case(k)
    wrong, _, _, _ = R.cg_half_epoch(c.mat, c.this, c.other, c.otor, 1e-12, 4 * k, variant="shift")
    rows = c.lens >= 2
    assert np.all(R.row_rel(wrong, c.x)[rows] > 10 * R.converged_bound(c.cond, 1e-7)[rows])


@pytest.mark.parametrize("k", R.KS)
def test_rounded_solution_is_below_the_warm_start_tolerance(k):
    "float32(x64) as warm start: r.r <= tol^2 y.y at tol = 1e-3, two orders to spare, in float32 too"
    c = R.case(k)
    x0 = c.x.astype(np.float32)
    for dtype in (np.float64, np.float32):
        x, its, frob, hists = R.cg_half_epoch(c.mat, x0, c.other, c.otor, 1e-3, 0, dtype)
        assert not its.any() and frob == 0.0 and np.array_equal(x.astype(np.float32), x0)
        for r, h in enumerate(hists):
            if h:
                s, e = c.mat.indptr[r], c.mat.indptr[r + 1]
                y = c.other[c.mat.indices[s:e]].astype(np.float64).T @ (c.mat.data[s:e] + 1.0)
                assert h[0] <= 1e-2 * 1e-6 * (y @ y)  # a relative residual of 1e-4 at the most


@pytest.mark.parametrize("k", [33, 256])
def test_not_spd_direction_of_the_failed_row_test(k):
    "otor = -1e6 I, other = ones, v = 1, x0 = 0: p is parallel to ones and p.Ap < 0"
    for n in (1, R.resident(R.padded(k)) + 1):
        A, y, dinv = R.row_system(np.ones((n, k)), np.ones(n), -1e6 * np.eye(k))
        p = y * dinv
        assert p @ (A @ p) < 0 and np.allclose(p, p[0])
