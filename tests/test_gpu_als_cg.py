"""GPU: the CG half-epoch (csrc/als_cg.hip, ``solver="cg"``) at every row-length seam of its two
instances against the NumPy restatement of the same loop (tests/als_cg_restatement.py): after a
fixed number of iterations, converged, by its iteration count, from a warm start at the answer,
through the task-control path and on a row it has to report.  The matrix, its seams and the
conditions these bounds rest on: ``seam_matrix`` and tests/test_als_cg_host.py."""
import numpy as np
import pytest

import als_cg_restatement as R

pytestmark = pytest.mark.gpu

K_IS64 = [(k, is64) for k in R.KS for is64 in (False, True)]


def _limit(mode, kp):
    "the longest row CG takes under LK_ALS_CG_HYBRID = mode"
    return {2: 16384 // kp, 1: 2048, 0: 1 << 40}[mode]


class _Run:
    "a CG plan over a case's matrix, its uploaded inputs, and one half-epoch at a time"

    def __init__(self, gpu, c, is64=False, ctl=None):
        import torch

        from lkpy_amd import _device as D
        from lkpy_amd import _native

        self.D, self.c, self.gpu = D, c, gpu
        dt = np.int64 if is64 else np.int32
        csr = D.DeviceCSR.from_arrays(c.mat.indptr.astype(dt), c.mat.indices, c.mat.data,
                                      c.mat.shape, gpu)
        assert csr.is64 == is64
        self.plan = D.ALSPlan(csr, c.k, _native.SOLVER_CG)
        assert self.plan.solver == _native.SOLVER_CG and self.plan.kp == c.kp
        if ctl is not None:
            self.plan.set_ctl(ctl)
        self.d_other = D.to_device_padded(c.other.copy(), gpu)  # (the shared case is read-only)
        self.d_otor = torch.from_numpy(c.otor.copy()).to(gpu)

    def __call__(self, tol, max_iter, this=None):
        "-> (rows [n x k] float32, frob, (iterations, rows by CG), the padded device rows)"
        this = self.c.this if this is None else this
        self.plan.set_cg(tol, max_iter)
        d_this = self.D.to_device_padded(this.copy(), self.gpu)
        frob = self.plan.half_epoch(d_this, self.d_other, self.d_otor)
        self.plan.check_status()
        got = self.D.to_host_unpadded(d_this, self.c.k)
        return got, float(frob.item()), self.plan.cg_stats(), d_this


def _check_fixed(run, negative, m, rows, tag):
    "exactly m iterations on the rows CG solved"
    c = run.c
    got, _frob, stats, _ = run(1e-20, m)
    n_cg = int(rows.sum())
    assert stats == (m * n_cg, n_cg), (tag, m, stats, n_cg)
    x64, _x32, e32_rows = R.fixed_iterations(c.k, negative, m)
    e32 = float(e32_rows[rows].max())
    dist = R.row_rel(got, x64)
    bound = R.fixed_bound(e32)
    worst = int(np.argmax(np.where(rows, dist, 0.0)))
    ratio = float(dist[worst] / bound)
    print(f"\ncg fixed {tag} m {m}: {n_cg} rows by CG, e32 {e32:.2e}, worst row distance "
          f"{dist[worst]:.2e} (length {c.lens[worst]}) = {ratio:.2f} of the bound")
    bad = np.flatnonzero(rows & ~(dist <= bound))
    assert bad.size == 0, (tag, m, [(int(c.lens[r]), float(dist[r])) for r in bad], bound)
    assert not got[c.lens == 0].any()


def _check_converged(run, rows_cg, tag):
    "tol = 1e-7: every row, the exact kernels' included -> the rows"
    c = run.c
    got, frob, stats, d_this = run(1e-7, 2 * c.k)
    assert stats[1] == int(rows_cg.sum())
    err = R.row_rel(got, c.x)
    bound = R.converged_bound(c.cond, 1e-7)
    nz = c.lens > 0
    worst = int(np.argmax(np.where(nz, err / bound, 0.0)))
    print(f"\ncg converged {tag}: {stats[1]} rows by CG, {stats[0]} iterations, worst row error "
          f"{err[worst]:.2e} (length {c.lens[worst]}) = {err[worst] / bound[worst]:.2f} of the bound")
    bad = np.flatnonzero(nz & ~(err <= bound))
    assert bad.size == 0, (tag, [(int(c.lens[r]), float(err[r]), float(bound[r])) for r in bad])
    assert (~nz).sum() == 3 and not got[~nz].any()  # implicit.rs:98-101
    if d_this.shape[1] > c.k:
        assert float(d_this[:, c.k:].abs().max().item()) == 0.0
    want_frob = R.frob_of(c.mat, got, c.this)  # (over the rows with entries, as the reference)
    assert abs(frob - want_frob) <= 1e-5 * want_frob, (frob, want_frob)
    got2, frob2, stats2, _ = run(1e-7, 2 * c.k)
    assert np.array_equal(got2, got) and frob2 == frob and stats2 == stats
    return got


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("k,is64", K_IS64)
def test_fixed_iterations(gpu, monkeypatch, k, is64, negative, mode):
    """`set_cg(1e-20, m)`, m = 1, 2, 3: every CG row takes exactly m iterations (an integer identity
    on the status words) and is within 4 e32 + 1e-6 of the float64 restatement after the same m
    iterations from the same warm start -- e32 = the float32 NumPy restatement's own largest row
    distance from float64.  Nothing has converged yet, so a wrong y, diagonal, warm start, alpha
    or beta shows at every share shape and tail length (tests/test_als_cg_host.py: a value paired
    with the next entry moves a row by 2.8e-2 or more).

    Measured: e32 (float32 NumPy against float64) = 1.8e-7 ... 3.2e-6 over all cases, the largest
    at k = 200, m = 3.  MI355X: the worst row of a case at 0.15 ... 0.65 of its bound -- 0.65 at
    k = 200, 0.54 at k = 256, 0.51 at k = 129, 0.42 at k = 128, at most 0.35 at k <= 100."""
    monkeypatch.setenv("LK_ALS_CG_HYBRID", str(mode))
    c = R.case(k, negative)
    run = _Run(gpu, c, is64)
    rows = (c.lens > 0) & (c.lens <= _limit(mode, c.kp))
    assert rows.sum() == {2: 34, 1: 50, 0: 52}[mode]
    for m in (1, 2, 3):
        _check_fixed(run, negative, m, rows,
                     f"k {k} is64 {int(is64)} neg {int(negative)} mode {mode}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k,is64", K_IS64)
def test_converged(gpu, monkeypatch, k, is64, mode):
    """`set_cg(1e-7, 2 k)`: every row -- those the exact kernels took too -- within
    cond (tol + 16 u) + 2e-6 of the float64 solve of the same system; empty rows and pad columns
    exactly zero; frob = sqrt(sum ||got - this0||^2) over the rows with entries (an empty row is
    zeroed and reports 0, as the reference's: implicit.rs:98-101) to 1e-5; bit-reproducible.
    Measured on an MI355X: the worst row at 0.02 ... 0.49 of its bound (0.49: a 1-entry row at
    k = 200, 1.25e-5 from float64; at most 0.21 at the other widths)."""
    monkeypatch.setenv("LK_ALS_CG_HYBRID", str(mode))
    c = R.case(k)
    _check_converged(_Run(gpu, c, is64), (c.lens > 0) & (c.lens <= _limit(mode, c.kp)),
                     f"k {k} is64 {int(is64)} mode {mode}")


@pytest.mark.parametrize("k,is64", K_IS64)
def test_iteration_totals(gpu, monkeypatch, k, is64):
    """`set_cg(1e-3, 2 k)` on every row: the iteration total lies between the float64 restatement's
    at 1.1e-3 and at 1e-3 / 1.1.  r.r is four orders above float32 round-off there; without the
    Jacobi diagonal the total is 1.8 x and more (tests/test_als_cg_host.py)."""
    monkeypatch.setenv("LK_ALS_CG_HYBRID", "0")
    c = R.case(k)
    lo, hi = R.iteration_totals(k, False, 1.1e-3), R.iteration_totals(k, False, 1e-3 / 1.1)
    _got, _frob, (its, rows), _ = _Run(gpu, c, is64)(1e-3, 2 * k)
    print(f"\ncg iterations k {k} is64 {int(is64)}: {its} on {rows} rows, float64 {lo} .. {hi}")
    assert rows == int((c.lens > 0).sum())
    assert lo <= its <= hi, (lo, its, hi)


@pytest.mark.parametrize("k,is64", K_IS64)
def test_warm_start_at_the_answer(gpu, monkeypatch, k, is64):
    """From the float64 solution rounded to float32 (true relative residual ~ cond u, far below
    tol = 1e-3; max_iter = 0 = k): no iteration on any row, the rows come back bit for bit,
    frob = 0."""
    monkeypatch.setenv("LK_ALS_CG_HYBRID", "0")
    c = R.case(k)
    x0 = c.x.astype(np.float32)
    got, frob, stats, _ = _Run(gpu, c, is64)(1e-3, 0, this=x0)
    assert stats == (0, int((c.lens > 0).sum()))
    assert np.array_equal(got.view(np.uint32), x0.view(np.uint32))
    assert frob == 0.0


@pytest.mark.parametrize("k,is64", K_IS64)
def test_task_control_path(gpu, monkeypatch, k, is64):
    """With a control block every row goes through the workgroup-per-row instance whatever its
    length and none to the exact kernels: rows of 1 ... RI entries meet the four-wave shares (waves
    that hold a partial group of 8, or nothing).  The fixed-iteration and converged checks again;
    a cancel before the launch leaves the rows untouched and the plan usable."""
    monkeypatch.delenv("LK_ALS_CG_HYBRID", raising=False)
    from lkpy_amd import _device as D

    c = R.case(k)
    ctl = D.TaskCtl()
    run = _Run(gpu, c, is64, ctl)
    rows = c.lens > 0
    tag = f"k {k} is64 {int(is64)} ctl"
    for m in (1, 2):
        _check_fixed(run, False, m, rows, tag)
        assert ctl.progress() == (c.n_rows, c.n_rows)
    want = _check_converged(run, rows, tag)
    assert ctl.progress() == (c.n_rows, c.n_rows)

    ctl.cancel()
    run.plan.set_cg(1e-7, 2 * k)
    d_this = D.to_device_padded(c.this.copy(), gpu)
    run.plan.half_epoch(d_this, run.d_other, run.d_otor)
    with pytest.raises(KeyboardInterrupt):
        run.plan.check_status()
    assert np.array_equal(D.to_host_unpadded(d_this, k).view(np.uint32), c.this.view(np.uint32))
    ctl.reset()
    run.plan.half_epoch(d_this, run.d_other, run.d_otor)
    run.plan.check_status()
    assert ctl.progress() == (c.n_rows, c.n_rows)
    assert np.array_equal(D.to_host_unpadded(d_this, k), want)


@pytest.mark.parametrize("instance", [1, 4])
@pytest.mark.parametrize("k", R.KS)
def test_failed_row_is_reported(gpu, monkeypatch, k, instance):
    """otor = -1e6 I, other = ones, values 1, this = 0: p is parallel to ones and
    p.Ap = |p|^2 (n k - 1e6) < 0, which CG reports like the Cholesky kernels report a failed pivot
    (test_gpu_als.py::test_not_spd_reports_error).  One row of 1 entry (wave-per-row instance) or
    of RI + 1 entries (workgroup-per-row instance)."""
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    monkeypatch.delenv("LK_ALS_CG_HYBRID", raising=False)
    n = 1 if instance == 1 else R.resident(R.padded(k)) + 1
    csr = D.DeviceCSR.from_arrays(np.array([0, n], np.int64), np.arange(n, dtype=np.int32),
                                  np.ones(n, np.float32), (1, n), gpu)
    plan = D.ALSPlan(csr, k, _native.SOLVER_CG)
    d_this = D.to_device_padded(np.zeros((1, k), np.float32), gpu)
    d_other = D.to_device_padded(np.ones((n, k), np.float32), gpu)
    plan.half_epoch(d_this, d_other, -1e6 * torch.eye(k, device=gpu))
    with pytest.raises(RuntimeError, match="ALS solve error"):
        plan.check_status()
    assert plan.cg_stats() == (0, 1)
