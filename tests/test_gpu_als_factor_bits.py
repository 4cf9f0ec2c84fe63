"""
The per-row code of the k <= 64 solve (csrc/als_chol.hip ``hybrid_step``, ``hybrid_solve``,
``LPack``: extraction, the 64 columns, the transposition, the rank-4 updates and the two
substitutions).  Taking vector instructions out of it may not move a bit, nor
change the status word or the error a failed row raises.

``tests/golden/als_factor_bits.json`` holds SHA-256 of the factor rows, of |d| and of the status
word that the commit BEFORE that change computed for the cases below;
``tools/record_factor_bits.py`` wrote it from the input builders of this file.  Every case is one
half-epoch over 300 columns from seeded, SIGNED factors.

Rows: 201 (no multiple of the four rows of a solve workgroup), of 0, 1, 3, 4, 5, 15, 16, 17, 63,
64, 65 and 130 entries in turn.  Widths 64, 50 (padded to 64), 32 and 10 (padded to 16): every lane
mask of the factorisation has a seam at each of them.  Two features are zero in every factor row:
their pivots sit at the regulariser alone.

The failing rows put the first non-positive pivot into column 0, 3 (last of a panel), 4 (first of
a panel) and 63 of the factorisation at k = 64: a NaN that travels through a lane the masks are
meant to discard would change what these half-epochs leave behind.
"""
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from test_gpu_als_solve_bits import ENV, REG, _hashes

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "als_factor_bits.json"
N_COLS = 300
SEAMS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130)
N_ROWS = 201
LENS = tuple(SEAMS[r % len(SEAMS)] for r in range(N_ROWS))
LENS_K128 = (17, 63, 64, 40, 33, 17, 64)  # als_wb64_kernel: 32 x 32 and 64 x 64 systems
ZERO_FEATURES = (2, 7)
KS = (64, 50, 32, 10)
BAD_ROW = 21  # 64 entries
BAD_COLUMNS = (0, 3, 4, 63)


@lru_cache(maxsize=None)
def _csr(lens=LENS):
    "(indptr, indices, values, shape), seeded"
    rng = np.random.default_rng(6300 + len(lens))
    cols, vals = [], []
    for n in lens:
        cols.append(np.sort(rng.choice(N_COLS, n, replace=False)).astype(np.int32))
        vals.append(rng.uniform(1.0, 40.0, n).astype(np.float32))
    indptr = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=indptr[1:])
    return indptr, np.concatenate(cols), np.concatenate(vals), (len(lens), N_COLS)


@lru_cache(maxsize=None)
def _factors(k, n_rows=N_ROWS):
    rng = np.random.default_rng(733 + k)
    P0 = rng.standard_normal((n_rows, k)).astype(np.float32) * 0.1
    Q0 = rng.standard_normal((N_COLS, k)).astype(np.float32) * 0.1
    Q0[:, list(ZERO_FEATURES)] = 0.0
    return P0, Q0


def _plan(dev, k, order, csr_arrays):
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    indptr, indices, values, shape = csr_arrays
    csr = D.DeviceCSR.from_arrays(indptr, indices, values, shape, dev)
    return D.ALSPlan(csr, k, _native.SOLVER_CHOLESKY, reference_order=order)


def half_epoch(dev, k, order="auto", explicit=False, lens=LENS):
    "one half-epoch from the seeded factors -> the hashes the golden file records"
    from lkpy_amd import _device as D

    plan = _plan(dev, k, order, _csr(lens))
    P0, Q0 = _factors(k, len(lens))
    P, Q = D.to_device_padded(P0, dev), D.to_device_padded(Q0, dev)
    if explicit:
        d = plan.half_epoch_explicit(P, Q, REG)
    else:
        d = plan.half_epoch(P, Q, D.Gramian(k, dev)(Q, REG))
    plan.check_status()
    return _hashes(plan, P, d, k)


def column_feature(c, k=64):
    "the feature that column c of the factorisation holds (tile c >> 4, sub c & 15)"
    nt = -(-k // 16)
    return (c & 15) * nt + (c >> 4)


def bad_pivot(dev, column, k=64):
    """One half-epoch in which exactly one row fails, its first non-positive pivot in ``column`` of
    the factorisation: the row's first entry names a column of the matrix whose factor row is the
    unit vector of that feature, with confidence -1e6.  The leading minors left of it are those of
    a positive definite matrix.  The error's text, the row it names and the hashes of what the
    half-epoch left behind."""
    from lkpy_amd import _device as D

    indptr, indices, values, shape = _csr()
    values = values.copy()
    lo = int(indptr[BAD_ROW])
    P0, Q0 = _factors(k)
    Q0 = Q0.copy()
    Q0[indices[lo]] = 0.0
    Q0[indices[lo], column_feature(column, k)] = 1.0
    values[lo] = -1.0e6
    plan = _plan(dev, k, "auto", (indptr, indices, values, shape))
    P, Q = D.to_device_padded(P0, dev), D.to_device_padded(Q0, dev)
    d = plan.half_epoch(P, Q, D.Gramian(k, dev)(Q, REG))
    try:
        plan.check_status()
        message = None
    except RuntimeError as e:
        message = str(e)
    return {"error": message, "row": BAD_ROW, **_hashes(plan, P, d, k)}


def k128_hashes(dev):
    "padded k = 128, rows of 17 .. 64 entries through als_wb64_kernel (LK_ALS_WB_MIN_ROWS=1)"
    return half_epoch(dev, 128, lens=LENS_K128)


def _cases():
    c = {}
    for k in KS:
        for order in ("auto", "accurate"):
            c[f"k{k}/implicit-{order}"] = lambda dev, k=k, o=order: half_epoch(dev, k, order=o)
            c[f"k{k}/explicit-{order}"] = lambda dev, k=k, o=order: half_epoch(dev, k, order=o,
                                                                               explicit=True)
    for col in BAD_COLUMNS:
        c[f"k64/bad-pivot-{col}"] = lambda dev, col=col: bad_pivot(dev, col)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture()
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_inputs_are_what_the_cases_need():
    assert N_ROWS % 4 != 0 and set(LENS) == set(SEAMS) and LENS[BAD_ROW] == 64
    assert 200 <= N_ROWS <= 210 and max(SEAMS) < N_COLS <= 400
    _, Q0 = _factors(64)
    assert (Q0 < 0).any() and (Q0 > 0).any() and not Q0[:, list(ZERO_FEATURES)].any()
    assert [column_feature(c) for c in BAD_COLUMNS] == [0, 12, 16, 63]
    assert not set(ZERO_FEATURES) & {column_feature(c) for c in BAD_COLUMNS}
    assert max(LENS_K128) <= 64 and min(LENS_K128) > 16


def test_golden_file_names_every_case(golden):
    assert set(golden) == set(CASES) | {"k128/woodbury64"}


@pytest.mark.parametrize("case", sorted(c for c in CASES if "/bad-" not in c))
def test_half_epoch_keeps_the_parent_bits(gpu, clean_env, golden, case):
    got = CASES[case](gpu)
    print(f"{case}: {got}")
    assert got == golden[case]


@pytest.mark.parametrize("column", BAD_COLUMNS)
def test_bad_pivot_raises_what_it_raised(gpu, clean_env, golden, column):
    got = bad_pivot(gpu, column)
    print(f"k64/bad-pivot-{column}: {got}")
    assert got["error"] is not None and "ALS solve error" in got["error"]
    assert f"row {got['row']} " in got["error"]
    assert got == golden[f"k64/bad-pivot-{column}"]


def test_k128_woodbury_rows_keep_the_parent_bits(gpu, clean_env, golden):
    clean_env.setenv("LK_ALS_WB_MIN_ROWS", "1")
    plan = _plan(gpu, 128, "auto", _csr(LENS_K128))
    assert plan.use_wb and plan.woodbury_rows == len(LENS_K128)
    got = k128_hashes(gpu)
    print(f"k128: {got}")
    assert got == golden["k128/woodbury64"]
