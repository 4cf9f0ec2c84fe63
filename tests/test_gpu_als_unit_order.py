"""
The order of the long rows' work units (``lk_als_plan_order_units``): the unit
table of a padded k <= 64 plan listed band by band per XCD instead of row by row.  Only the table
moves -- slabs, slab groups, the row order and every sum stay -- so no result may change by a bit.

* The inputs of ``tests/test_gpu_als_chunk_units.py`` (its builders, imported) with ordered plans,
  at every forced unit size, through the half-epoch and the epoch call: the hashes that
  ``tests/golden/als_chunk_bits.json`` records of the commit before the chunk-unit work.
* Small matrices of 300 columns with ``LK_ALS_REF_LEN=256`` (rows of 257, 513, 1025 and 2052
  entries are long): 1, 3, 5, 9, 19 and 33 units (no multiples of 4; fewer than 8 workgroups; one
  more than 8 x 4), every unit starting at column 0, 64-bit offsets, a view with a row offset, a key
  map, no long row, the call made twice.  Each runs ordered against ``LK_ALS_UNIT_ORDER=0``.
* The table itself (``lk_als_plan_unit_table``): a permutation of the row-major one with (first
  entry, entries, slab) kept together; the units of XCD 0, 1, ... 7 (physical workgroup b on XCD
  b % 8), each along b, one behind the other ARE the list sorted by (key, row, first entry) --
  which is all of: keys ascending along b, consecutive runs, only the last workgroup partial.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from test_gpu_als_chunk_units import (ITEM_REG, USER_REG, _csr, _factors, _hashes, _setup,
                                      clean_env, golden)  # noqa: F401 -- fixtures

pytestmark = pytest.mark.gpu

N_XCD = 8
N_COLS = 300


@pytest.fixture()
def env(clean_env):
    clean_env.delenv("LK_ALS_UNIT_ORDER", raising=False)
    return clean_env


# ---- the recorded bits of the chunk-unit inputs ---------------------------------------------------

@pytest.mark.parametrize("k", [64, 50])
@pytest.mark.parametrize("unit", [None, 256, 512, 1024])
def test_ordered_half_epoch_keeps_the_recorded_bits(gpu, env, golden, k, unit):
    if unit is not None:
        env.setenv("LK_ALS_REF_UNIT", str(unit))
    plan, P, Q, qtq, _ = _setup(gpu, k, "auto")
    before = plan.unit_table()
    plan.order_units()
    assert _is_ordered(plan, before, _csr()[0], _csr()[1])
    d = plan.half_epoch(P, Q, qtq)
    plan.check_status()
    assert _hashes(P, d, k) == golden[f"k{k}"]["auto"]


@pytest.mark.parametrize("k", [64, 50])
def test_ordered_accurate_plan_keeps_the_recorded_bits(gpu, env, golden, k):
    plan, P, Q, qtq, _ = _setup(gpu, k, "accurate")
    plan.order_units()
    d = plan.half_epoch(P, Q, qtq)
    plan.check_status()
    assert _hashes(P, d, k) == golden[f"k{k}"]["accurate"]


def _epoch(dev, k, unit, ordered, env):
    "(hashes of the user side, Q, |dQ|, the two Gramians) of one lk_als_implicit_epoch"
    import torch

    from lkpy_amd import _device as D

    if unit is not None:
        env.setenv("LK_ALS_REF_UNIT", str(unit))
    u_plan, P, Q, qtq, gram = _setup(dev, k, "auto")
    indptr, indices, values, shape = _csr()
    iu = sps.csr_array(sps.csr_array((values, indices, indptr), shape=shape).T)
    iu.sum_duplicates()
    i_plan = D.ALSPlan(D.DeviceCSR.from_scipy(iu, dev), k, reference_order="auto")
    if ordered:
        u_plan.order_units()
        i_plan.order_units()
    ptp = torch.empty_like(qtq)
    delta = torch.empty(2, dtype=torch.float32, device=dev)
    D.als_implicit_epoch(u_plan, i_plan, P, Q, qtq, USER_REG, ptp, ITEM_REG, gram, delta)
    u_plan.check_status()
    i_plan.check_status()
    return _hashes(P, delta[0], k), [t.cpu().numpy() for t in (Q, delta, qtq, ptp)]


@pytest.mark.parametrize("k", [64, 50])
@pytest.mark.parametrize("unit", [None, 256, 512, 1024])
def test_ordered_epoch_call_keeps_the_bits(gpu, env, golden, k, unit):
    "user side: the recorded hashes; item side and both Gramians: the unordered run's bits"
    user, rest = _epoch(gpu, k, unit, True, env)
    assert user == golden[f"k{k}"]["auto"]
    env.setenv("LK_ALS_UNIT_ORDER", "0")
    user0, rest0 = _epoch(gpu, k, unit, True, env)
    assert user0 == user
    for a, b in zip(rest, rest0):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the table -----------------------------------------------------------------------------------

def _is_ordered(plan, before, indptr, indices, key_map=None):
    "is the plan's table the row-major table `before`, sorted and dealt as the header says?"
    beg, length, slab = plan.unit_table()
    n = len(beg)
    b_beg, b_len, b_slab = before
    # (first entries are distinct: every unit has entries of its own)
    at = np.argsort(b_beg)
    assert np.array_equal(np.sort(beg), b_beg[at])
    pos = np.searchsorted(b_beg[at], beg)
    assert np.array_equal(length, b_len[at][pos]) and np.array_equal(slab, b_slab[at][pos])
    col = np.asarray(indices)[beg]
    key = col if key_map is None else key_map[col]
    row = np.searchsorted(np.asarray(indptr, dtype=np.int64), beg, side="right") - 1
    n_wg = (n + 3) // 4
    walk = [u for x in range(N_XCD) for b in range(x, n_wg, N_XCD)
            for u in range(4 * b, min(4 * b + 4, n))]
    assert sorted(walk) == list(range(n))
    want = np.lexsort((beg, row, key))
    return np.array_equal(np.asarray(walk, dtype=np.int64), want)


SMALL = {
    # name: (long rows, LK_ALS_REF_UNIT, k, units)
    "one_unit": ((257,), 1024, 64, 1),
    "three_units": ((513,), 256, 64, 3),
    "five_units": ((1025,), 256, 64, 5),
    "nine_units": ((2052,), 256, 64, 9),
    "nineteen_units_k32": ((2052, 257, 1025, 513), None, 32, 19),
    "thirty_three_units": ((2052, 1025, 257, 2052, 513, 1025), 256, 64, 33),
    "units_of_512": ((2052, 1025, 257, 2052, 513, 1025), 512, 64, 19),
}


def _small_csr(long, seed=5, n_short=9, first_col_zero=False, dtype=np.int32):
    "long rows (columns drawn with replacement: 300 columns) among short ones, seeded"
    rng = np.random.default_rng(seed)
    lens = [int(n) for n in rng.integers(0, 41, n_short)]
    for j, n in enumerate(long):
        lens.insert(2 * j + 1, n)
    cols, vals = [], []
    for n in lens:
        c = np.sort(rng.integers(0, N_COLS, n)).astype(np.int32)
        if first_col_zero:
            c[::256] = 0
        cols.append(c)
        vals.append(rng.uniform(1.0, 40.0, n).astype(np.float32))
    indptr = np.zeros(len(lens) + 1, dtype)
    np.cumsum(lens, out=indptr[1:])
    return indptr, np.concatenate(cols), np.concatenate(vals), (len(lens), N_COLS)


def _run(dev, csr, k, ordered_with=None, rows=None, check=None):
    """one half-epoch of the matrix (or of its rows [lo, hi): a view with a row offset), the plan
    ordered by ``ordered_with(plan)``; -> bits of the factors, of |d|, and the unit count"""
    from lkpy_amd import _device as D
    from lkpy_amd import _native

    indptr, indices, values, shape = csr
    mat = D.DeviceCSR.from_arrays(indptr, indices, values, shape, dev)
    if rows is not None:
        lo, hi = rows
        mat = D.DeviceCSR(mat.indptr[lo : hi + 1], mat.indices, mat.values, (hi - lo, shape[1]),
                          mat.h_indptr[lo : hi + 1])
    plan = D.ALSPlan(mat, k, reference_order="auto")
    before = plan.unit_table()
    if ordered_with is not None:
        ordered_with(plan)
        if check is not None:
            check(plan, before, mat.h_indptr)
    rng = np.random.default_rng(11)
    P = D.to_device_padded((rng.standard_normal((mat.shape[0], k)).astype(np.float32) * 0.1) ** 2,
                           dev)
    Q = D.to_device_padded((rng.standard_normal((shape[1], k)).astype(np.float32) * 0.1) ** 2, dev)
    d = plan.half_epoch(P, Q, D.Gramian(k, dev)(Q, USER_REG))
    plan.check_status()
    units = int(_native.load().lk_als_plan_units(plan._h))
    return P.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32), units


def _ordered_equals_unordered(dev, env, csr, k, unit, units=None, key_map=None, rows=None,
                              twice=False):
    import torch

    env.setenv("LK_ALS_REF_LEN", "256")
    if unit is not None:
        env.setenv("LK_ALS_REF_UNIT", str(unit))
    seen = {}

    def order(plan):
        key = None if key_map is None else torch.from_numpy(key_map.astype(np.int32)).to(dev)
        plan.order_units(key)
        if twice:
            first = plan.unit_table()
            plan.order_units(key)
            assert all(np.array_equal(a, b) for a, b in zip(first, plan.unit_table()))

    def check(plan, before, h_indptr):
        seen["ordered"] = _is_ordered(plan, before, h_indptr, csr[1], key_map)
        seen["moved"] = not np.array_equal(before[0], plan.unit_table()[0])

    got = _run(dev, csr, k, order, rows, check)
    assert seen["ordered"]
    if units is not None:
        assert got[2] == units
    env.setenv("LK_ALS_UNIT_ORDER", "0")
    off = _run(dev, csr, k, order, rows,
               lambda plan, before, _: seen.update(
                   kept=all(np.array_equal(a, b) for a, b in zip(before, plan.unit_table()))))
    assert seen["kept"]  # the switch keeps the row-major table
    plain = _run(dev, csr, k, None, rows)
    for a, b, c in zip(got[:2], off[:2], plain[:2]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    return seen


@pytest.mark.parametrize("name", list(SMALL))
def test_small_plans_ordered_against_unordered(gpu, env, name):
    long, unit, k, units = SMALL[name]
    seen = _ordered_equals_unordered(gpu, env, _small_csr(long), k, unit, units)
    assert seen["moved"] or len(long) == 1  # (one row in few workgroups: sorted as it stands)


def test_equal_keys(gpu, env):
    "every unit starts at column 0: the order falls back to (row, offset), dealt per XCD"
    csr = _small_csr((2052, 1025, 257, 2052, 513, 1025), first_col_zero=True)
    _ordered_equals_unordered(gpu, env, csr, 64, 256, 33)


def test_offsets_of_64_bits(gpu, env):
    csr = _small_csr((2052, 1025, 257, 2052, 513, 1025), dtype=np.int64)
    _ordered_equals_unordered(gpu, env, csr, 64, 256, 33)


def test_view_with_a_row_offset(gpu, env):
    "rows [3, 13) of the matrix, the offsets not rebased (as the sharded engine hands them in)"
    csr = _small_csr((2052, 1025, 257, 2052, 513, 1025))
    lens = np.diff(csr[0])[3:13]
    units = int(sum((n + 255) // 256 for n in lens if n > 256))
    assert units not in (0, 33)
    _ordered_equals_unordered(gpu, env, csr, 64, 256, units, rows=(3, 13))


def test_key_map(gpu, env):
    "the band of a unit read through a column map (a relabelled matrix: original-of-new)"
    csr = _small_csr((2052, 1025, 257, 2052, 513, 1025))
    key_map = np.random.default_rng(3).permutation(N_COLS).astype(np.int64)
    _ordered_equals_unordered(gpu, env, csr, 64, 256, 33, key_map=key_map)


def test_called_twice(gpu, env):
    csr = _small_csr((2052, 1025, 257, 2052, 513, 1025))
    _ordered_equals_unordered(gpu, env, csr, 64, 256, 33, twice=True)


def test_no_long_row(gpu, env):
    "nothing to order: the call succeeds and the table is empty"
    got = _ordered_equals_unordered(gpu, env, _small_csr(()), 64, None, 0)
    assert not got["moved"]


def test_wider_plans_are_left_alone(gpu, env):
    "padded k = 128: als_blk.hip's chunk launch reads the table in row-major order"
    from lkpy_amd import _device as D

    env.setenv("LK_ALS_REF_LEN", "256")
    indptr, indices, values, shape = _small_csr((2052, 1025, 513))
    plan = D.ALSPlan(D.DeviceCSR.from_arrays(indptr, indices, values, shape, gpu), 128,
                     reference_order="auto")
    before = plan.unit_table()
    plan.order_units()
    assert len(before[0]) > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, plan.unit_table()))


# ---- LK_ALS_PLAN_BAND_UNITS: a unit per block for the plans whose units are ordered ---------------

def _plan_unit(lens, flags, k=64):
    import ctypes

    from lkpy_amd import _native

    lib = _native.require_gpu()
    indptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    h = ctypes.c_void_p(0)
    rc = lib.lk_als_plan_create_ex(ctypes.byref(h), indptr.ctypes.data_as(ctypes.c_void_p), 1,
                                   len(lens), k, _native.SOLVER_CHOLESKY, flags)
    assert rc == 0, _native.last_error()
    try:
        return int(lib.lk_als_plan_unit(h)), int(lib.lk_als_plan_units(h))
    finally:
        lib.lk_als_plan_destroy(h)


def test_band_units_flag_takes_a_unit_per_block(gpu, env):
    many = np.full(4000, 4096)  # enough long rows for the 1024-entry units of the default rule
    assert _plan_unit(many, 2) == (1024, 16000)
    assert _plan_unit(many, 2 | 4) == (256, 64000)
    # (plans that are not hybrid, or wider, ignore the flag)
    assert _plan_unit(many, 4) == _plan_unit(many, 0)
    assert _plan_unit(many, 2 | 4, k=128) == _plan_unit(many, 2, k=128)
    env.setenv("LK_ALS_REF_UNIT", "512")
    assert _plan_unit(many, 2 | 4) == (512, 32000)  # the variable still wins
    env.delenv("LK_ALS_REF_UNIT")
    env.setenv("LK_ALS_UNIT_ORDER", "0")
    assert _plan_unit(many, 2 | 4) == (1024, 16000)  # today's order keeps today's rule


@pytest.mark.parametrize("k", [64, 50])
def test_band_units_plan_keeps_the_recorded_bits(gpu, env, golden, k):
    from lkpy_amd import _device as D

    indptr, indices, values, shape = _csr()
    plan = D.ALSPlan(D.DeviceCSR.from_arrays(indptr, indices, values, shape, gpu), k,
                     reference_order="auto", band_units=True)
    plan.order_units()
    _, P, Q, qtq, _ = _setup(gpu, k, "auto")
    d = plan.half_epoch(P, Q, qtq)
    plan.check_status()
    assert _hashes(P, d, k) == golden[f"k{k}"]["auto"]
