"""
``lk_als_implicit_epoch`` (csrc/als_chol.hip ``als_chol_epoch``): one native call
per epoch that schedules the two halves' small kernels off the critical path.  It launches the
same kernels as the per-half calls, so everything it produces is BIT FOR BIT what

    plan.half_epoch(user) ; Gramian(P) ; plan.half_epoch(item) ; Gramian(Q)

produces: P, Q, both Gramians, |dP|, |dQ| and the reference-order right-hand sides of the long
rows.  Every value is read with ``.cpu()`` on the current stream and NO device synchronisation in
between: a missing join between the call's side streams and the launch stream shows as a
difference.

``LK_ALS_REF_LEN=256`` makes "long" start at 257 entries, so that a matrix of a thousand rows has
every path: one-unit long rows, rows of several slabs over two work units, rows of 1 and 2 entries,
empty rows and columns, a half without any long row (no fork), and plans without a chunk at all.
(A row of more than 1024 entries needs more than 1024 columns: the matrix is 1400 x 1200.)
"""
import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

EPOCHS = 3


def _matrix(seed, n_users, n_items, long_rows=(), long_cols=(), bg=40):
    """seeded 0/1 pattern: every user 0 .. bg random items, then users 0.. get ``long_rows``
    entries and items 0.. ``long_cols``; users / items 10 .. 14 empty, users 15, 16 one entry,
    users 17, 18 two"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n_users, n_items), dtype=bool)
    for u in range(n_users):
        m[u, rng.choice(n_items, int(rng.integers(0, bg + 1)), replace=False)] = True
    for u, n in enumerate(long_rows):
        m[u] = False
        m[u, rng.choice(n_items, n, replace=False)] = True
    for i, n in enumerate(long_cols):
        m[:, i] = False
        m[rng.choice(n_users, n, replace=False), i] = True
    m[10:15] = False
    m[:, 10:15] = False
    for u, n in ((15, 1), (16, 1), (17, 2), (18, 2)):
        m[u] = False
        m[u, 20 + rng.choice(n_items - 20, n, replace=False)] = True
    ui = sps.csr_array(m.astype(np.float32))
    ui.data = rng.uniform(1.0, 40.0, ui.nnz).astype(np.float32)
    ui.sort_indices()
    return ui


BOTH_SIDES = dict(seed=5, n_users=1400, n_items=1200, long_rows=(1100, 600, 450, 300),
                  long_cols=(1150, 580, 420, 310))
USER_SIDE = dict(seed=6, n_users=1400, n_items=1200, long_rows=(1100, 600, 450, 300))
NO_LONG = dict(seed=7, n_users=200, n_items=150, bg=30)


def _engines(gpu, spec, k, monkeypatch):
    "two engines from the same seeded start; plans built with LK_ALS_REF_LEN=256"
    from lkpy_amd._als_engine import HipBackend, ImplicitALSEngine

    monkeypatch.setenv("LK_ALS_REF_LEN", "256")
    monkeypatch.delenv("LK_ALS_RHS_ORDER", raising=False)
    ui = _matrix(**spec)
    rng = np.random.default_rng(spec["seed"] + 100)
    Q0 = (rng.standard_normal((ui.shape[1], k)).astype(np.float32) * 0.01) ** 2
    P0 = (rng.standard_normal((ui.shape[0], k)).astype(np.float32) * 0.01) ** 2
    return ui, [ImplicitALSEngine(ui, k, 0.1, 0.05, P0, Q0, HipBackend(k, gpu)) for _ in range(2)]


def _old_epoch(eng):
    "the epoch as the per-half calls run it: half_epoch + Gramian per half"
    b = eng.backend
    du = eng.u_plan.half_epoch(eng.P, eng.Q, eng._qtq).clone()
    ptp = b.gramian(eng.P, eng.item_reg)
    di = eng.i_plan.half_epoch(eng.Q, eng.P, ptp).clone()
    eng._qtq = b.gramian(eng.Q, eng.user_reg)
    return du, di, ptp


def _bits(t):
    "the raw bits of a device tensor, read on the current stream (no device synchronisation)"
    return t.cpu().numpy().view(np.uint32)


def _state(eng, du, di, ptp):
    out = {"P": _bits(eng.P), "Q": _bits(eng.Q), "qtq": _bits(eng._qtq), "ptp": _bits(ptp),
           "dP": _bits(du.reshape(1)), "dQ": _bits(di.reshape(1))}
    for name, plan in (("yref_u", eng.u_plan), ("yref_i", eng.i_plan)):
        y = plan.yref_tasks()
        if y is not None and y.numel() > 0:
            out[name] = _bits(y)
    return out


def _compare_epochs(new, old, native: bool):
    assert new._native_epoch() == native
    for epoch in range(EPOCHS):
        du, di = new.train_epoch()
        got = _state(new, du, di, new._ptp if native else new.backend.gramian(new.P, new.item_reg))
        want = _state(old, *_old_epoch(old))
        assert got.keys() == want.keys()
        for key in want:
            assert np.array_equal(got[key], want[key]), (epoch, key)
        assert np.isfinite(got["dP"].view(np.float32)).all()
    new.check()
    old.check()
    return want


@pytest.mark.parametrize("k", [64, 50, 32, 10])
def test_epoch_call_matches_the_half_epoch_calls(gpu, monkeypatch, k):
    "long rows and long columns: both halves fork, chunk, chain, sum slabs and solve long rows"
    ui, (new, old) = _engines(gpu, BOTH_SIDES, k, monkeypatch)
    for plan in (new.u_plan, new.i_plan):
        lens = np.diff(plan.csr.h_indptr)
        # (one row of several slabs over two 1024-entry work units, three one-unit long rows)
        assert lens.max() > 1024 and (lens == 0).sum() >= 5
        assert plan.long_rows() == 4 == int((lens > 256).sum())
    assert {1, 2} <= set(np.diff(new.u_plan.csr.h_indptr).tolist())
    want = _compare_epochs(new, old, native=True)
    assert "yref_u" in want and "yref_i" in want


def test_epoch_call_with_long_rows_on_one_side_only(gpu, monkeypatch):
    "the item half has no long row: no fork there, the user half's tail still runs beside it"
    ui, (new, old) = _engines(gpu, USER_SIDE, 64, monkeypatch)
    assert new.u_plan.long_rows() == 4 and new.i_plan.long_rows() == 0
    assert np.diff(new.i_plan.csr.h_indptr).max() <= 256
    want = _compare_epochs(new, old, native=True)
    assert "yref_u" in want and "yref_i" not in want


def test_epoch_call_without_any_long_row(gpu, monkeypatch):
    "n_y = 0 and n_chunks = 0 in both halves"
    ui, (new, old) = _engines(gpu, NO_LONG, 64, monkeypatch)
    assert new.u_plan.long_rows() == 0 and new.i_plan.long_rows() == 0
    _compare_epochs(new, old, native=True)


def test_engine_keeps_the_half_epoch_calls_at_k128(gpu, monkeypatch):
    "padded k = 128 is not served by the epoch call: train_epoch runs the per-half path"
    from lkpy_amd import _device as D

    ui, (new, old) = _engines(gpu, NO_LONG, 128, monkeypatch)
    assert not D.epoch_plans_ok(new.u_plan, new.i_plan)
    _compare_epochs(new, old, native=False)
    assert getattr(new, "_ptp", None) is None
