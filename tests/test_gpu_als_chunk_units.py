"""
The long-row chunk kernel of the k <= 64 ALS half-epoch (csrc/als_chol.hip ``als_chunk_kernel``,
DESIGN.md 4.1c): plans whose chunked rows all take their right-hand side from the reference-order
chains run it without the y arithmetic, and hybrid plans at padded k = 64 choose the entries per
work unit (1024 / 512 / 256) at creation.  Neither may move a bit: summation order, slab
boundaries and the y chains are what they were.

``tests/golden/als_chunk_bits.json`` holds SHA-256 of the factor rows and of |d| that the commit
BEFORE these changes computed for the inputs below (one ``lk_als_implicit_half_epoch`` from seeded
factors, default plan, and the same with an ``accurate``-order plan, which keeps y in the chunk
kernel).  Every run here must reproduce them.

Inputs: 6 000 columns, 60 short rows (0 .. 40 entries) and nine long rows -- 2049 (the shortest long
row, twice: the number of long rows is no multiple of the four rows of a solve workgroup), 2304 and
2560 (whole blocks; a 1024-entry unit remainder of one and of two blocks), 3073 and 4100 (a last
block of one and of four entries), 4352 (17 whole blocks), 9000 and 20 000.  4100 and above have
more than 16 blocks.  The rows of 9000 and 20 000 entries are longer than the matrix is wide: their
columns are drawn with replacement (a CSR row may name a column twice; the kernels sum entries).
"""
import ctypes
import hashlib
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "als_chunk_bits.json"
N_COLS = 6000
LONG = (2049, 2304, 2560, 3073, 4100, 4352, 9000, 20000, 2049)
N_SHORT = 60
USER_REG, ITEM_REG = 0.1, 0.05


@lru_cache(maxsize=None)
def _csr():
    "(indptr, indices, values, shape): the long rows spread among the short ones, seeded"
    rng = np.random.default_rng(20240)
    lens = [int(n) for n in rng.integers(0, 41, N_SHORT)]
    lens[3], lens[7], lens[11] = 0, 1, 2
    for j, n in enumerate(LONG):
        lens.insert(5 + 7 * j, n)
    cols, vals = [], []
    for n in lens:
        c = rng.choice(N_COLS, n, replace=False) if n <= N_COLS else rng.integers(0, N_COLS, n)
        cols.append(np.sort(c).astype(np.int32))
        vals.append(rng.uniform(1.0, 40.0, n).astype(np.float32))
    indptr = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=indptr[1:])
    return indptr, np.concatenate(cols), np.concatenate(vals), (len(lens), N_COLS)


@lru_cache(maxsize=None)
def _factors(k):
    rng = np.random.default_rng(77 + k)
    n_rows, n_cols = _csr()[3]
    P0 = (rng.standard_normal((n_rows, k)).astype(np.float32) * 0.1) ** 2
    Q0 = (rng.standard_normal((n_cols, k)).astype(np.float32) * 0.1) ** 2
    return P0, Q0


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hashes(P, d, k):
    from lkpy_amd import _device as D

    return {"rows": _sha(D.to_host_unpadded(P, k)),
            "d": _sha(d.reshape(1).cpu().numpy().astype(np.float32))}


def _setup(dev, k, order):
    "(plan of the matrix, P, Q, Q^T Q + reg I, the Gramian object) on the device"
    from lkpy_amd import _device as D

    indptr, indices, values, shape = _csr()
    plan = D.ALSPlan(D.DeviceCSR.from_arrays(indptr, indices, values, shape, dev), k,
                     reference_order=order)
    P0, Q0 = _factors(k)
    P, Q = D.to_device_padded(P0, dev), D.to_device_padded(Q0, dev)
    gram = D.Gramian(k, dev)
    return plan, P, Q, gram(Q, USER_REG), gram


def half_epoch_hashes(dev, k, order):
    "one lk_als_implicit_half_epoch from the seeded factors (what the golden file records)"
    plan, P, Q, qtq, _ = _setup(dev, k, order)
    d = plan.half_epoch(P, Q, qtq)
    plan.check_status()
    return _hashes(P, d, k)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ("LK_ALS_REF_UNIT", "LK_ALS_RHS_ORDER", "LK_ALS_REF_LEN", "LK_ALS_SIDE_STREAM"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_inputs_are_what_the_cases_need():
    indptr = _csr()[0]
    lens = np.diff(indptr)
    long = lens[lens > 2048]
    assert sorted(long.tolist()) == sorted(LONG) and len(long) % 4 != 0
    assert (lens <= 40).sum() == N_SHORT and (lens == 0).any() and (lens == 1).any()


@pytest.mark.parametrize("k", [64, 50])
@pytest.mark.parametrize("unit", [None, 256, 512, 1024])
def test_half_epoch_keeps_the_parent_bits(gpu, clean_env, golden, k, unit):
    "default plan (the unit chosen at creation) and every forced unit: the parent's bits"
    if unit is not None:
        clean_env.setenv("LK_ALS_REF_UNIT", str(unit))
    got = half_epoch_hashes(gpu, k, "auto")
    print(f"k={k} unit={unit}: {got}")
    assert got == golden[f"k{k}"]["auto"]


@pytest.mark.parametrize("k", [64, 50])
def test_accurate_order_keeps_its_parent_bits(gpu, clean_env, golden, k):
    "an accurate-order plan forms y in the chunk kernel as before"
    got = half_epoch_hashes(gpu, k, "accurate")
    print(f"k={k} accurate: {got}")
    assert got == golden[f"k{k}"]["accurate"]


@pytest.mark.parametrize("k", [64, 50])
def test_epoch_call_keeps_the_parent_bits_on_the_user_side(gpu, clean_env, golden, k):
    "lk_als_implicit_epoch: P and |dP| of its user half are the half-epoch call's"
    import torch

    from lkpy_amd import _device as D

    u_plan, P, Q, qtq, gram = _setup(gpu, k, "auto")
    indptr, indices, values, shape = _csr()
    iu = sps.csr_array(sps.csr_array((values, indices, indptr), shape=shape).T)
    iu.sum_duplicates()
    i_plan = D.ALSPlan(D.DeviceCSR.from_scipy(iu, gpu), k, reference_order="auto")
    assert D.epoch_plans_ok(u_plan, i_plan)
    ptp = torch.empty_like(qtq)
    delta = torch.empty(2, dtype=torch.float32, device=gpu)
    P_in = P.clone()
    D.als_implicit_epoch(u_plan, i_plan, P, Q, qtq, USER_REG, ptp, ITEM_REG, gram, delta)
    u_plan.check_status()
    i_plan.check_status()
    got = _hashes(P, delta[0], k)
    print(f"k={k} epoch call, user side: {got}")
    assert got == golden[f"k{k}"]["auto"]
    assert not torch.equal(P, P_in) and bool(torch.isfinite(delta).all())


def _plan_units(lens, k=64):
    "(entries per work unit, work units) of a default plan built from row lengths alone"
    from lkpy_amd import _native

    lib = _native.require_gpu()
    indptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    h = ctypes.c_void_p(0)
    rc = lib.lk_als_plan_create_ex(ctypes.byref(h), indptr.ctypes.data_as(ctypes.c_void_p), 1,
                                   len(lens), k, _native.SOLVER_CHOLESKY, 2)
    assert rc == 0, _native.last_error()
    try:
        return int(lib.lk_als_plan_unit(h)), int(lib.lk_als_plan_units(h))
    finally:
        lib.lk_als_plan_destroy(h)


def test_unit_is_chosen_by_the_number_of_units(gpu, clean_env):
    "few long rows: a unit per 256-entry block; many: the 1024-entry units; the variable wins"
    few = np.diff(_csr()[0])
    blocks = int(sum((n + 255) // 256 for n in few if n > 2048))
    assert _plan_units(few) == (256, blocks)
    many = np.full(4000, 4096)  # 16 000 units of 1024 entries: twice the chunk waves of 390 CUs
    assert _plan_units(many) == (1024, 16000)
    clean_env.setenv("LK_ALS_REF_UNIT", "512")
    assert _plan_units(few)[0] == 512 and _plan_units(many) == (512, 32000)
    clean_env.setenv("LK_ALS_REF_UNIT", "1024")
    assert _plan_units(few)[0] == 1024
    clean_env.delenv("LK_ALS_REF_UNIT")
    assert _plan_units(few, k=32)[0] == 256  # (narrower plans: a unit is a block, as before)
