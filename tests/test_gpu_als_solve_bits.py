"""
The k <= 64 solve kernel of the ALS half-epoch (csrc/als_chol.hip ``als_solve_kernel``, its Gram
loop and ``hybrid_solve``) and the two kernels that share code with it -- the
long-row chunk kernel (the Gram loop) and ``als_wb64_kernel`` at padded k = 128 (``hybrid_solve``
and the L image).  Cutting vector instructions out of them may not move a bit.

``tests/golden/als_solve_bits.json`` holds SHA-256 of the factor rows, of |d| and of the status
word that the commit BEFORE that change computed for the cases below; ``tools/record_solve_bits.py``
wrote it from the input builders of this file.  Every case is one half-epoch from seeded factors.

Inputs: 4 000 columns; one row of each length at the seams of the Gram loop -- 0 .. 5 (masked last
group), 31 .. 33 (the 8-group ring fills exactly), 63 .. 65 (batch boundary), 95 .. 97 (the first
length at which the unguarded batch loop runs: 16 + 8 groups), 127 .. 129, 200, 255 .. 257, 2047,
2048 (the longest short row) and 2049 (one long row: the chunk kernel and the YREF solve launch
run).  25 rows: no multiple of the four rows of a solve workgroup.
"""
import hashlib
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "als_solve_bits.json"
N_COLS = 4000
LENS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257,
        2047, 2048, 2049)
LENS_K128 = (17, 40, 64, 17, 40, 64, 33)  # als_wb64_kernel: 32 x 32 and 64 x 64 systems
KS = (64, 50, 40, 32, 10)
REG = 0.1
ENV = ("LK_ALS_REF_UNIT", "LK_ALS_RHS_ORDER", "LK_ALS_REF_LEN", "LK_ALS_SIDE_STREAM",
       "LK_ALS_WB_MIN_ROWS", "LK_ALS_WB64_K128", "LK_ALS_WB64")


@lru_cache(maxsize=None)
def _csr(lens=LENS, wide=False):
    "(indptr, indices, values, shape), seeded; ``wide``: 64-bit row offsets"
    rng = np.random.default_rng(4100 + len(lens))
    cols, vals = [], []
    for n in lens:
        cols.append(np.sort(rng.choice(N_COLS, n, replace=False)).astype(np.int32))
        vals.append(rng.uniform(1.0, 40.0, n).astype(np.float32))
    indptr = np.zeros(len(lens) + 1, np.int64 if wide else np.int32)
    np.cumsum(lens, out=indptr[1:])
    return indptr, np.concatenate(cols), np.concatenate(vals), (len(lens), N_COLS)


@lru_cache(maxsize=None)
def _factors(k, n_rows=len(LENS)):
    rng = np.random.default_rng(177 + k)
    P0 = (rng.standard_normal((n_rows, k)).astype(np.float32) * 0.1) ** 2
    Q0 = (rng.standard_normal((N_COLS, k)).astype(np.float32) * 0.1) ** 2
    return P0, Q0


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hashes(plan, P, d, k):
    from lkpy_amd import _device as D

    import torch

    status = plan.ws[:4].view(torch.int32).cpu().numpy()  # (the workspace begins with it)
    return {"rows": _sha(D.to_host_unpadded(P, k)),
            "d": _sha(d.reshape(1).cpu().numpy().astype(np.float32)),
            "status": _sha(status)}


def _setup(dev, k, order, lens=LENS, wide=False):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    indptr, indices, values, shape = _csr(lens, wide)
    csr = D.DeviceCSR.from_arrays(indptr, indices, values, shape, dev)
    assert csr.is64 == wide
    plan = D.ALSPlan(csr, k, _native.SOLVER_CHOLESKY, reference_order=order)
    P0, Q0 = _factors(k, len(lens))
    P, Q = D.to_device_padded(P0, dev), D.to_device_padded(Q0, dev)
    return plan, P, Q, D.Gramian(k, dev)


def half_epoch(dev, k, order="auto", explicit=False, wide=False, ctl=False, lens=LENS):
    "one half-epoch from the seeded factors -> the hashes the golden file records"
    from lkpy_amd import _device as D

    plan, P, Q, gram = _setup(dev, k, order, lens, wide)
    block = None
    if ctl:
        block = D.TaskCtl()
        plan.set_ctl(block)
    d = plan.half_epoch_explicit(P, Q, REG) if explicit else plan.half_epoch(P, Q, gram(Q, REG))
    plan.check_status()
    if ctl:
        assert block.progress() == (len(lens), len(lens))
    return _hashes(plan, P, d, k)


def epoch_call(dev, k):
    "lk_als_implicit_epoch over the matrix and its transpose -> hashes of both sides"
    import torch

    from lkpy_amd import _device as D

    u_plan, P, Q, gram = _setup(dev, k, "auto")
    indptr, indices, values, shape = _csr()
    iu = sps.csr_array(sps.csr_array((values, indices, indptr), shape=shape).T)
    i_plan = D.ALSPlan(D.DeviceCSR.from_scipy(iu, dev), k, reference_order="auto")
    assert D.epoch_plans_ok(u_plan, i_plan)
    qtq = gram(Q, REG)
    ptp = torch.empty_like(qtq)
    delta = torch.empty(2, dtype=torch.float32, device=dev)
    D.als_implicit_epoch(u_plan, i_plan, P, Q, qtq, REG, ptp, REG, gram, delta)
    u_plan.check_status()
    i_plan.check_status()
    return {"user": _hashes(u_plan, P, delta[0], k), "item": _hashes(i_plan, Q, delta[1], k)}


def not_spd(dev, k=64):
    """a row whose normal matrix is not positive definite (confidence values far below zero):
    the error's text, and the hashes of what the half-epoch left behind"""
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    indptr, indices, values, shape = _csr()
    values = values.copy()
    bad = LENS.index(33)
    values[indptr[bad]:indptr[bad + 1]] = -1.0e6
    plan = D.ALSPlan(D.DeviceCSR.from_arrays(indptr, indices, values, shape, dev), k,
                     _native.SOLVER_CHOLESKY, reference_order="auto")
    P0, Q0 = _factors(k)
    P, Q = D.to_device_padded(P0, dev), D.to_device_padded(Q0, dev)
    d = plan.half_epoch(P, Q, D.Gramian(k, dev)(Q, REG))
    try:
        plan.check_status()
        message = None
    except RuntimeError as e:
        message = str(e)
    return {"error": message, "row": bad, **_hashes(plan, P, d, k)}


def _cases():
    c = {}
    for k in KS:
        c[f"k{k}/implicit"] = lambda dev, k=k: half_epoch(dev, k)
        c[f"k{k}/explicit"] = lambda dev, k=k: half_epoch(dev, k, explicit=True)
        c[f"k{k}/accurate"] = lambda dev, k=k: half_epoch(dev, k, order="accurate")
        c[f"k{k}/accurate-explicit"] = lambda dev, k=k: half_epoch(dev, k, order="accurate",
                                                                   explicit=True)
        c[f"k{k}/wide-offsets"] = lambda dev, k=k: half_epoch(dev, k, wide=True)
        c[f"k{k}/task-control"] = lambda dev, k=k: half_epoch(dev, k, ctl=True)
    c["k64/reference"] = lambda dev: half_epoch(dev, 64, order="reference")
    c["k64/epoch-call"] = lambda dev: epoch_call(dev, 64)
    c["k64/not-spd"] = lambda dev: not_spd(dev)
    return c


CASES = _cases()


def k128_hashes(dev):
    "padded k = 128, rows of 17 / 40 / 64 entries through als_wb64_kernel (LK_ALS_WB_MIN_ROWS=1)"
    return half_epoch(dev, 128, lens=LENS_K128)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_inputs_are_what_the_cases_need():
    assert len(LENS) % 4 != 0 and sum(n > 2048 for n in LENS) == 1
    for seam in (4, 32, 64, 96, 128, 256, 2048):
        assert {seam - 1, seam, seam + 1} <= set(LENS)
    assert {0, 1, 2, 3, 4, 5, 200} <= set(LENS)
    assert {17, 40, 64} <= set(LENS_K128) and max(LENS_K128) <= 64 and min(LENS_K128) > 16


def test_golden_file_names_every_case(golden):
    assert set(golden) == set(CASES) | {"k128/woodbury64"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_half_epoch_keeps_the_parent_bits(gpu, clean_env, golden, case):
    got = CASES[case](gpu)
    print(f"{case}: {got}")
    assert got == golden[case]


def test_not_spd_row_still_raises(gpu, clean_env, golden):
    got = not_spd(gpu)
    assert got["error"] is not None and "ALS solve error" in got["error"]
    assert f"row {got['row']} " in got["error"]
    assert got == golden["k64/not-spd"]


def test_k128_woodbury_rows_keep_the_parent_bits(gpu, clean_env, golden):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    clean_env.setenv("LK_ALS_WB_MIN_ROWS", "1")
    indptr, indices, values, shape = _csr(LENS_K128)
    plan = D.ALSPlan(D.DeviceCSR.from_arrays(indptr, indices, values, shape, gpu), 128,
                     _native.SOLVER_CHOLESKY)
    assert plan.use_wb and plan.woodbury_rows == len(LENS_K128)
    got = k128_hashes(gpu)
    print(f"k128: {got}")
    assert got == golden["k128/woodbury64"]


def test_gather_addresses_past_4_gib(gpu, clean_env):
    """The k = 64 Gram loop gathers with 32-bit byte offsets only from tables smaller than 4 GiB
    (decided per launch on the host).  A table of 2^24 + 8 padded rows (4.3 GB, uninitialised but
    for the rows used) is past that: one 8-entry row naming columns on both sides of row 2^24
    must come out bit for bit as from a small table holding the same eight rows.  (Offsets cut to
    32 bits would fetch rows 0 .. 7 for the columns past 2^24: those hold other numbers.)"""
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd import _native

    k, big = 64, (1 << 24) + 8
    assert big * k * 4 >= 1 << 32 > (big - 9) * k * 4
    cols = np.array([8, 4097, (1 << 24) - 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 6,
                     (1 << 24) + 7], np.int64)
    vals = np.random.default_rng(5).uniform(1.0, 40.0, len(cols)).astype(np.float32)
    rows = torch.from_numpy(_factors(k)[1][: len(cols)].copy()).to(gpu)
    otor = D.Gramian(k, gpu)(D.to_device_padded(_factors(k)[1], gpu), REG)

    def solve(n_cols, indices, table):
        indptr = np.array([0, len(indices)], np.int32)
        csr = D.DeviceCSR.from_arrays(indptr, indices.astype(np.int32), vals, (1, n_cols), gpu)
        plan = D.ALSPlan(csr, k, _native.SOLVER_CHOLESKY, reference_order="auto")
        this = torch.zeros((1, k), dtype=torch.float32, device=gpu)
        d = plan.half_epoch(this, table, otor)
        plan.check_status()
        return this.cpu().numpy(), float(d)

    small = torch.zeros((len(cols), k), dtype=torch.float32, device=gpu)
    small.copy_(rows)
    want, d_want = solve(len(cols), np.arange(len(cols)), small)
    table = torch.empty((big, k), dtype=torch.float32, device=gpu)
    table[:8] = 1.0
    table[torch.from_numpy(cols).to(gpu)] = rows
    got, d_got = solve(big, cols, table)
    del table
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and d_got == d_want
