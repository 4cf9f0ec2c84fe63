"""
Device-resident implicit-ALS training engine (one process per GPU).

Mirrors the epoch structure of ``ALSTrainerBase`` / ``ImplicitMFTrainer``
(src/lenskit/als/_common.py:209-256, src/lenskit/als/_implicit.py:135-175):

    epoch = user half (OtOr = Q^T Q + user_reg I, previous Q)
          + item half (OtOr = P^T P + item_reg I, NEW P)

but keeps both CSR orientations and both factor matrices in HBM across epochs, so a
training run crosses PCIe once in and once out.

Row layout.  Users and items are RELABELLED once at set-up: rows are sorted by length
(longest first) and dealt round-robin to the ``world`` ranks; rank r owns the
contiguous block ``[r*rpr, (r+1)*rpr)`` of the relabelled matrix (padded with empty
rows).  This gives every rank the same row count and nearly the same nnz, lets the
half-epoch kernel write straight into the rank's slice of the replicated factor
matrix, makes the exchange a single in-place ``all_gather_into_tensor`` (RCCL picks
the xGMI full-mesh all-gather), and packs the factor rows of popular items together
(better L2 hit rate for the gathers).  Host-visible factors are un-permuted on
download, so callers never see the relabelling.

Collectives per epoch (world > 1): all-gather of the freshly solved P slice, k x k
all-reduce of the slice Gramians, the same for Q, and a scalar all-reduce of the
squared deltas.  No collective at world == 1.

Overlap (world > 1).  The gathered rows of a half-epoch are needed only by the NEXT half, so a
rank's rows are cut into ``slices`` (LK_ALS_OVERLAP_SLICES; automatic: 4 for factor matrices of
256 MB and more, else 1) equal blocks and the
relabelling interleaves them -- new row = slice * (world * m) + rank * m + j -- so that slice s
of ALL ranks is one contiguous super-block: the half-epoch runs slice by slice (one plan per
slice), and the in-place all-gather of super-block s is issued asynchronously right behind the
solve of slice s, i.e. it travels over xGMI while slice s + 1 is being solved; the k x k slice
Gramians of the rank's own rows are formed meanwhile too.  Only the last slice's gather is
exposed.  (cfg5 at 8 GPUs: 10 GB of user factors per half-epoch, as long on the links as the
solve takes.)  The slices share one Z = other @ OtOr^-1 (ALSPlanGroup).

The arithmetic lives behind a small backend object so the sharding / exchange logic
can be exercised on CPU (gloo) in tests with the oracle standing in for the kernels;
the product backend is :class:`HipBackend` and there is no fallback.
"""

from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sps
import torch
import torch.distributed as dist

from . import _native


def deal_rows(lengths: np.ndarray, world: int, slices: int = 1, keep_order: bool = False,
              order: np.ndarray | None = None):
    """
    Relabelling of rows for ``world`` ranks: returns (new_of_old, old_of_new, rpr) with
    ``rpr`` rows per rank.  The j-th row dealt to ``rank`` goes to slice j % slices of that rank;
    with m = rpr / slices rows per (rank, slice) block, new index =
    slice * (world * m) + rank * m + j // slices -- for slices == 1: rank * rpr + j.
    Slots beyond the real rows (padding) have old_of_new == -1.
    ``keep_order`` (one rank, one slice): the identity -- the strict reference-order mode, where
    the ORDER OF A ROW'S ENTRIES (= ascending label of the other side) is part of the arithmetic
    (the reference's sequential float32 sums run over it).  ``order``: the rows by descending
    length, ties in row order, when the caller has it already (the engine sorts on the device:
    NumPy's stable argsort of 10^7 lengths is 1-4 s of a 1.1 s set-up... on the host alone).
    """
    n = len(lengths)
    if keep_order:
        assert world == 1 and slices == 1
        ident = np.arange(n, dtype=np.int64)
        return ident, ident.copy(), n
    if order is None:
        order = np.argsort(-lengths.astype(np.int64), kind="stable")
    rpr = (n + world - 1) // world
    m = (rpr + slices - 1) // slices
    rpr = m * slices
    j, r = np.divmod(np.arange(n), world)
    # serpentine dealing keeps the per-rank nnz closer than plain round-robin
    r = np.where(j % 2 == 0, r, world - 1 - r)
    new_pos = (j % slices) * (world * m) + r * m + j // slices
    new_of_old = np.empty(n, dtype=np.int64)
    new_of_old[order] = new_pos
    old_of_new = np.full(world * rpr, -1, dtype=np.int64)
    old_of_new[new_pos] = order
    return new_of_old, old_of_new, rpr


def _relabel_csr(mat: sps.csr_array, row_new_of_old, n_rows_new, col_new_of_old, n_cols_new):
    "Apply the row/column relabelling; returns CSR with sorted column indices."
    coo = mat.tocoo()
    out = sps.csr_array(
        (coo.data, (row_new_of_old[coo.row], col_new_of_old[coo.col])),
        shape=(n_rows_new, n_cols_new),
    )
    out.sort_indices()
    return out


def shard_local_blocks(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                       u_old: np.ndarray, u_new: np.ndarray, i_new: np.ndarray,
                       u_blocks, i_blocks, by_new_user: bool):
    """
    Per-rank set-up (``LK_ALS_SETUP=sharded``): the rows THIS rank solves, in both orientations,
    cut out of the original CSR without ever forming the relabelled matrix or its transpose in
    full.  Plain torch on whatever device the arrays live on (HBM in the product, host tensors in
    the gloo tests), so the same code is exercised on CPU:

    * user side: the rank's user rows (``u_blocks``: ranges of NEW row numbers; ``u_old[new]`` =
      original row or -1 for padding) gathered in dealt order, columns mapped by ``i_new``, the
      order of a row's entries kept -- what ``lk_csr_relabel`` does for all rows;
    * item side: ONE pass over the entries keeps those whose new item number falls into
      ``i_blocks`` (nnz / world of them), their original user comes from a search in the offsets,
      and a stable sort by (local item row, user) lists every item row's entries by ascending
      ORIGINAL user (``by_new_user=False``: the reference's order, _common.py:216-219) or by
      ascending new user (``True``: what the full stable transpose of the relabelled matrix gives
      in ``accurate`` mode); the user numbers are then relabelled by ``u_new``.

    What stays RESIDENT is nnz / world entries per orientation; the item-side pass itself holds
    three int64 temporaries of the size of the whole matrix for its duration (the widened indices,
    the mapped item numbers, the block search: ~24 B per entry, 2.4 GB at cfg5 -- ADVICE r5; not
    chunked: a set-up transient on a 288 GB device).

    Returns ``{"u": (h_ptr, ptr, idx, val), "i": (...)}``: offsets over the rank's rows in block
    order (host NumPy + device), int32 indices, float32 values -- entry for entry the rows
    ``make_plans_on_device`` would view out of the full matrices.
    """
    dev = indices.device
    n_u0 = len(u_new)
    ptr64 = indptr.to(torch.int64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)  # noqa: E731
    d_i_new = t(i_new, torch.int64)

    # ---- user side: gather the rank's rows
    rows_new = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in u_blocks])
    src_row = u_old[rows_new]  # original row, -1 = padding
    d_src = t(np.maximum(src_row, 0), torch.int64)
    lens = (ptr64[d_src + 1] - ptr64[d_src]) * t(src_row >= 0, torch.int64)
    u_ptr = torch.zeros(len(rows_new) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=u_ptr[1:])
    total = int(u_ptr[-1])
    # entry e of local row r sits at source position start[r] + (e - u_ptr[r])
    shift = torch.repeat_interleave(ptr64[d_src] - u_ptr[:-1], lens, output_size=total)
    pos = torch.arange(total, dtype=torch.int64, device=dev) + shift
    u_idx = d_i_new[indices[pos].to(torch.int64)].to(torch.int32)
    u_val = values[pos]

    # ---- item side: the entries of the rank's items, by (item row, user)
    ni = int(i_new.max()) + 1 if len(i_new) else 0
    ni = max(ni, max((hi for _, hi in i_blocks), default=0))
    loc_of_new = torch.full((ni,), -1, dtype=torch.int64, device=dev)
    rows_i = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in i_blocks])
    loc_of_new[t(rows_i, torch.int64)] = torch.arange(len(rows_i), dtype=torch.int64, device=dev)
    loc = loc_of_new[d_i_new[indices.to(torch.int64)]]
    sel = torch.nonzero(loc >= 0).flatten()  # ascending position = ascending original user
    loc = loc[sel]
    orig_user = torch.searchsorted(ptr64, sel, right=True) - 1
    user = t(u_new, torch.int64)[orig_user] if by_new_user else orig_user
    order = torch.sort(loc * max(n_u0, int(u_new.max()) + 1 if n_u0 else 1) + user,
                       stable=True).indices
    counts = torch.bincount(loc, minlength=len(rows_i))
    i_ptr = torch.zeros(len(rows_i) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=i_ptr[1:])
    i_idx = t(u_new, torch.int64)[orig_user[order]].to(torch.int32)
    i_val = values[sel[order]]
    return {"u": (u_ptr.cpu().numpy(), u_ptr, u_idx, u_val),
            "i": (i_ptr.cpu().numpy(), i_ptr, i_idx, i_val)}


def relabelled_user_lists(ui: sps.csr_array, u_old: np.ndarray, i_new: np.ndarray):
    """
    (offsets int64, items int32) of ALL user rows in the engine's row order with the engine's item
    numbers -- the exclusion lists of a top-N call on ``eng.P`` / ``eng.Q``.  With the default
    set-up every rank has them on the device (``eng.u_plan.csr.full_h_indptr`` / ``.indices``);
    with ``LK_ALS_SETUP=sharded`` no rank does, and whoever scores all users builds them here.
    """
    ui = sps.csr_array(ui)
    src = np.maximum(u_old, 0)
    lens = np.where(u_old >= 0, np.diff(ui.indptr)[src], 0).astype(np.int64)
    ptr = np.zeros(len(u_old) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    pos = np.arange(ptr[-1], dtype=np.int64) + np.repeat(ui.indptr[src].astype(np.int64) - ptr[:-1],
                                                         lens)
    return ptr, i_new[ui.indices[pos]].astype(np.int32)


def sharded_setup() -> bool:
    """With more than one rank every rank derives only its OWN rows from the one upload of the
    matrix (the default since round 6; bit-checked under gloo and with ranks as threads on one
    GPU); ``LK_ALS_SETUP=full`` (or ``replicated``): every rank relabels and transposes the full
    matrix, as rounds 1-5 did."""
    v = os.environ.get("LK_ALS_SETUP", "").strip().lower()
    if v in ("", "sharded"):
        return True
    if v in ("full", "replicated"):
        return False
    raise ValueError(f"unknown LK_ALS_SETUP {v!r} (sharded / full)")


def sharded_z() -> bool:
    "LK_ALS_Z=sharded: Z = other @ OtOr^-1 formed once across the ranks (default: on every rank)"
    v = os.environ.get("LK_ALS_Z", "").strip().lower()
    if v in ("", "replicated"):
        return False
    if v == "sharded":
        return True
    raise ValueError(f"unknown LK_ALS_Z {v!r} (replicated / sharded)")


class TorchComm:
    """The engine's collectives on ``torch.distributed`` (backend ``nccl`` = RCCL on the GPU boxes).

    ``enable_timing(True)``: every collective is bracketed by events on the current stream and
    ``timing_ms()`` returns the milliseconds spent per kind since the last call -- what a rank's
    stream WAITED for (a blocking collective: its whole duration; an asynchronous row gather:
    only what was still outstanding at ``wait()``, i.e. the part the solve of the next slice did
    not hide).  ``bench.py --gpus N`` prints it per rank beside the epoch time, so that the first
    multi-GPU run can be read against DESIGN.md section 6's predicted table.
    """

    def __init__(self, group=None):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self._timing = False
        self._events = []  # (kind, start, end)

    def enable_timing(self, on: bool = True):
        self._timing = bool(on)
        self._events = []

    def _timed(self, kind, fn):
        if not (self._timing and torch.cuda.is_available()):
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self._events.append((kind, a, b))
        return out

    def timing_ms(self) -> dict:
        "milliseconds per kind of collective since enable_timing / the last call (synchronises)"
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        tot = {}
        for kind, a, b in self._events:
            tot[kind] = tot.get(kind, 0.0) + float(a.elapsed_time(b))
        self._events = []
        return tot

    def broadcast(self, t: torch.Tensor):
        self._timed("broadcast", lambda: dist.broadcast(t, src=_global_rank(self.group, 0),
                                                        group=self.group))

    def all_reduce(self, t: torch.Tensor):
        self._timed("all_reduce", lambda: dist.all_reduce(t, op=dist.ReduceOp.SUM,
                                                          group=self.group))

    def all_gather_rows(self, full: torch.Tensor, lo: int, hi: int):
        "in place: every rank's row block [lo, hi) of ``full`` ends up in everybody's ``full``"
        self._timed("all_gather", lambda: dist.all_gather_into_tensor(full, full[lo:hi],
                                                                      group=self.group))

    def all_gather_block_async(self, full: torch.Tensor, slo: int, shi: int, lo: int, hi: int):
        """
        The same inside the super-block [slo, shi) (= the blocks [lo, hi) of all ranks, in rank
        order), ASYNCHRONOUS: the collective is ordered behind what the current stream holds now
        (the solve of these rows) and runs beside what is launched next; ``.wait()`` on the
        returned handle orders the current stream behind it.
        """
        h = dist.all_gather_into_tensor(full[slo:shi], full[lo:hi], group=self.group,
                                        async_op=True)
        if not self._timing:
            return h
        comm = self

        class _TimedHandle:
            def wait(self_inner):
                return comm._timed("all_gather_exposed_wait", h.wait)

        return _TimedHandle()


class LoopbackComm:
    """
    ``world`` ranks as THREADS of one process exchanging through shared memory -- the same
    collectives with the same semantics (rank-ordered sums, in-place row gather), so that the
    row-sharded engine can run with two or more ranks on ONE GPU (``tests/test_gpu_sharded.py``:
    the device relabelling with padding rows, the plan views with non-zero row offsets, the
    Woodbury buffers of a shard -- everything but the wire).  Not a transport: a test double.
    """

    class _Shared:
        def __init__(self, world):
            import threading

            self.world = world
            self.barrier = threading.Barrier(world)
            self.slots = [None] * world

    def __init__(self, shared: "LoopbackComm._Shared", rank: int):
        self.sh, self.rank, self.world, self.group = shared, rank, shared.world, None

    @staticmethod
    def make(world: int):
        sh = LoopbackComm._Shared(world)
        return [LoopbackComm(sh, r) for r in range(world)]

    def _sync_device(self, t):
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()

    def broadcast(self, t):
        self._sync_device(t)
        self.sh.slots[self.rank] = t
        self.sh.barrier.wait()
        if self.rank != 0:
            t.copy_(self.sh.slots[0])
            self._sync_device(t)
        self.sh.barrier.wait()

    def all_reduce(self, t):
        self._sync_device(t)
        self.sh.slots[self.rank] = t.clone()
        self.sh.barrier.wait()
        acc = self.sh.slots[0].clone()
        for r in range(1, self.world):  # rank order, like a ring would not guarantee -- fixed here
            acc += self.sh.slots[r]
        self.sh.barrier.wait()
        t.copy_(acc)
        self._sync_device(t)

    def all_gather_rows(self, full, lo, hi):
        self._sync_device(full)
        self.sh.slots[self.rank] = (full[lo:hi], lo, hi)
        self.sh.barrier.wait()
        for r in range(self.world):
            if r != self.rank:
                src, a, b = self.sh.slots[r]
                full[a:b].copy_(src)
        self._sync_device(full)
        self.sh.barrier.wait()

    class _Done:
        def wait(self):
            return True

    def all_gather_block_async(self, full, slo, shi, lo, hi):
        "(test double: done by the time it returns)"
        self.all_gather_rows(full, lo, hi)
        return LoopbackComm._Done()


class HipBackend:
    "The product backend: hand-written HIP kernels through the C ABI."

    def __init__(self, k: int, dev, solver=_native.SOLVER_AUTO, reference_order=None):
        from . import _device as D

        self.D = D
        self.k = k
        self.dev = D.device(dev)
        self.kp = D.padded_dim(k)
        self.solver = solver
        # the order of the two long sums of a row (LK_ALS_RHS_ORDER): "auto" (the
        # default: rows of more than 2048 entries in the reference's own order), "reference"
        # (strict: every row of more than 256 entries), "accurate" (round 4's default); None =
        # what the process environment says
        self.order_mode = D.als_order_mode(reference_order)
        if solver == _native.SOLVER_CG or self.kp > 256:
            self.order_mode = "accurate"
        self.reference_order = self.order_mode == "reference"
        self._gram = D.Gramian(k, self.dev)

    def make_plan(self, local_csr: sps.csr_array):
        csr = self.D.DeviceCSR.from_scipy(local_csr, self.dev)
        return self.D.ALSPlan(csr, self.k, self.solver, reference_order=self.order_mode)

    def make_plans_on_device(self, ui, u_old, i_new, i_old, u_rng, i_rng, ilen=None):
        """
        Both orientations of the RELABELLED matrix built in HBM from one upload of the original
        CSR (``lk_csr_relabel`` + the stable device transpose ``lk_csr_transpose``) instead of
        SciPy COO round trips on the host (2.2 s of the 2.3 s set-up on ML-25M): rows gathered in
        dealt order, columns mapped, entry order inside a row kept (the row solve sums over a
        row's entries; any order).  Returns the plans of this rank's user rows ``u_rng`` and item
        rows ``i_rng`` -- views into the full device matrices, offsets not rebased.  ``u_rng`` /
        ``i_rng`` may be LISTS of ranges (the row slices of the overlapped half-epoch): the plans
        then come as one ``ALSPlanGroup`` per orientation.
        """
        D = self.D
        lib = _native.require_gpu()
        import ctypes

        dev = self.dev
        n_users, n_items = ui.shape
        nu, ni = len(u_old), len(i_old)
        if isinstance(ui, D.DeviceCSR):  # already resident (e.g. generated in HBM)
            src = ui
        else:
            src = D.DeviceCSR.from_arrays(ui.indptr, ui.indices, ui.data, ui.shape, dev)
        pdt = src.h_indptr.dtype
        ulen = np.diff(src.h_indptr)
        if ilen is None:
            ilen = np.bincount(ui.indices, minlength=n_items)
        new_ulen = np.where(u_old >= 0, ulen[np.maximum(u_old, 0)], 0)
        new_ilen = np.where(i_old >= 0, ilen[np.maximum(i_old, 0)], 0)
        h_uptr = np.zeros(nu + 1, dtype=pdt)
        np.cumsum(new_ulen, out=h_uptr[1:])
        h_iptr = np.zeros(ni + 1, dtype=pdt)
        np.cumsum(new_ilen, out=h_iptr[1:])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_uptr = to(h_uptr)
        nnz = src.nnz
        idx = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)[:nnz]
        # (named, not inline: a temporary tensor would be released -- and its block handed to the
        # next upload -- before the kernel that reads it is even launched)
        d_row_src = to(u_old.astype(np.int32))
        d_col_map = to(i_new.astype(np.int32))
        _native.check(lib.lk_csr_relabel(
            D._ptr(src.indptr), 1 if src.is64 else 0, D._ptr(src.indices), D._ptr(src.values), nu,
            D._ptr(d_row_src), D._ptr(d_uptr), D._ptr(d_col_map), D._ptr(idx), D._ptr(val),
            D._stream()), "lk_csr_relabel")
        ui_new = D.DeviceCSR(d_uptr, idx, val, (nu, ni), h_uptr)
        if self.order_mode == "accurate":
            iu_new = D.csr_transpose(ui_new)  # stable: entries of an item row by ascending new user
        else:
            # The reference sums a row's entries in the order its CSR lists them: ascending
            # ORIGINAL label of the other side (SciPy's tocsr / .T.tocsr, _common.py:216-219).
            # The user rows above keep that order (lk_csr_relabel maps the columns, it does not
            # sort them).  For the item rows the transposition starts from the ORIGINAL row order
            # -- rows not permuted, columns mapped -- so that the stable transpose lists an item's
            # entries by ascending original user; the user numbers are relabelled afterwards.  A
            # row's column indices are then not ascending: no ALS kernel needs them to be.
            n_u0 = src.shape[0]
            d_ident = torch.arange(n_u0, dtype=torch.int32, device=dev)
            idx0 = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
            val0 = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)[:nnz]
            _native.check(lib.lk_csr_relabel(
                D._ptr(src.indptr), 1 if src.is64 else 0, D._ptr(src.indices), D._ptr(src.values),
                n_u0, D._ptr(d_ident), D._ptr(src.indptr), D._ptr(d_col_map), D._ptr(idx0),
                D._ptr(val0), D._stream()), "lk_csr_relabel")
            ui_cm = D.DeviceCSR(src.indptr, idx0, val0, (n_u0, ni), src.h_indptr)
            iu_new = D.csr_transpose(ui_cm)  # rows = new items, entries by ascending ORIGINAL user
            d_u_new = torch.full((n_u0,), -1, dtype=torch.int32, device=dev)
            live = torch.from_numpy(np.flatnonzero(u_old >= 0).astype(np.int64)).to(dev)
            d_u_new[d_row_src[live].long()] = live.to(torch.int32)
            iu_new.indices = d_u_new[iu_new.indices.long()]
            iu_new.shape = (ni, nu)
            del ui_cm, idx0, val0, d_ident, d_u_new
        iu_new.h_indptr = h_iptr
        del src

        def local(full, h_ptr, lo, hi, n_cols):
            view = D.DeviceCSR(full.indptr[lo : hi + 1], full.indices, full.values,
                               (hi - lo, n_cols), h_ptr[lo : hi + 1])
            view.full_h_indptr = h_ptr  # offsets of ALL rows (every rank holds the full arrays)
            return D.ALSPlan(view, self.k, self.solver, reference_order=self.order_mode,
                             band_units=True)  # (order_units below)

        def plans(full, h_ptr, rngs, n_cols):
            if isinstance(rngs, tuple):
                return local(full, h_ptr, rngs[0], rngs[1], n_cols), \
                    int(h_ptr[rngs[1]] - h_ptr[rngs[0]])
            ps = [local(full, h_ptr, lo, hi, n_cols) for lo, hi in rngs]
            nnz_ = sum(int(h_ptr[hi] - h_ptr[lo]) for lo, hi in rngs)
            return (ps[0] if len(ps) == 1 else D.ALSPlanGroup(ps, n_cols)), nnz_

        up, unnz = plans(ui_new, h_uptr, u_rng, ni)
        ip, innz = plans(iu_new, h_iptr, i_rng, nu)
        return up, ip, (unnz, innz)

    def make_plans_sharded(self, ui, u_old, u_new, i_new, n_items_new, u_rng, i_rng):
        """
        ``LK_ALS_SETUP=sharded`` (world > 1): the plans of this rank's rows from arrays that hold
        ONLY this rank's rows -- one upload of the original CSR, then :func:`shard_local_blocks`
        (the user rows gathered, the item rows cut out of one pass over the entries and sorted):
        nothing of the size of the whole relabelled matrix or its transpose is built, the original
        is released, and what stays resident is nnz / world entries per orientation.  Same entry
        order per row as ``make_plans_on_device``; ``u_rng`` / ``i_rng`` as there.
        """
        D = self.D
        dev = self.dev
        if isinstance(ui, D.DeviceCSR):
            src = ui
        else:
            src = D.DeviceCSR.from_arrays(ui.indptr, ui.indices, ui.data, ui.shape, dev)
        ub = [u_rng] if isinstance(u_rng, tuple) else list(u_rng)
        ib = [i_rng] if isinstance(i_rng, tuple) else list(i_rng)
        out = shard_local_blocks(src.indptr, src.indices, src.values, u_old, u_new, i_new, ub, ib,
                                 by_new_user=self.order_mode == "accurate")
        pdt = src.h_indptr.dtype
        tdt = torch.int64 if pdt == np.int64 else torch.int32
        del src

        def plans(arrs, blocks, n_cols):
            h_ptr, d_ptr, idx, val = arrs
            h_ptr = h_ptr.astype(pdt)
            d_ptr = d_ptr.to(tdt)
            full = D.DeviceCSR(d_ptr, idx, val, (len(h_ptr) - 1, n_cols), h_ptr)
            ps, lo = [], 0
            for b_lo, b_hi in blocks:  # the rank's blocks lie one behind the other in its arrays
                hi = lo + (b_hi - b_lo)
                view = D.DeviceCSR(full.indptr[lo : hi + 1], full.indices, full.values,
                                   (hi - lo, n_cols), h_ptr[lo : hi + 1])
                view.full_h_indptr = None  # no rank holds the offsets of all rows
                ps.append(D.ALSPlan(view, self.k, self.solver, reference_order=self.order_mode,
                                    band_units=True))  # (order_units below)
                lo = hi
            return (ps[0] if len(ps) == 1 else D.ALSPlanGroup(ps, n_cols)), int(h_ptr[-1])

        up, unnz = plans(out["u"], ub, n_items_new)
        ip, innz = plans(out["i"], ib, len(u_old))
        return up, ip, (unnz, innz)

    def order_units(self, u_plans, i_old, i_plans, u_old):
        """
        Once per plan at set-up (padded k <= 64): the long rows' work units band
        by band per XCD.  The plans of ``make_plans_on_device`` / ``make_plans_sharded`` list a
        row's entries by ascending ORIGINAL label of the other side, so a unit's band is the
        original label of its first column (``accurate`` order: item rows ascend by new user).
        """
        if self.kp > 64:
            return  # (the plans' band_units flag does nothing there either)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)  # noqa: E731
        i_key = to(i_old)
        for p in u_plans:
            p.order_units(i_key)
        u_key = None if self.order_mode == "accurate" else to(u_old)
        for p in i_plans:
            p.order_units(u_key)

    def upload(self, mat: np.ndarray) -> torch.Tensor:
        return self.D.to_device_padded(mat, self.dev)

    def upload_permuted(self, mat: np.ndarray, new_of_old: np.ndarray, n_new: int) -> torch.Tensor:
        "[n_new x KP] device matrix with row new_of_old[i] = mat[i] (other rows zero)"
        src = self.D.to_device_padded(np.ascontiguousarray(mat, dtype=np.float32), self.dev)
        out = torch.zeros((n_new, src.shape[1]), dtype=torch.float32, device=self.dev)
        out.index_copy_(0, torch.from_numpy(np.asarray(new_of_old, dtype=np.int64)).to(self.dev),
                        src)
        return out

    def random_init(self, n: int, old_of_new: np.ndarray, seed: int) -> torch.Tensor:
        "[n x KP] factors ~ (N(0,1) * 0.01)^2 drawn on the device; padding rows / columns zero"
        g = torch.Generator(device=self.dev)
        g.manual_seed(seed)
        m = torch.zeros((n, self.kp), dtype=torch.float32, device=self.dev)
        m[:, : self.k] = (torch.randn((n, self.k), generator=g, device=self.dev) * 0.01) ** 2
        if (old_of_new < 0).any():
            m[torch.from_numpy(np.flatnonzero(old_of_new < 0)).to(self.dev)] = 0.0
        return m

    def download(self, mat: torch.Tensor) -> np.ndarray:
        return self.D.to_host_unpadded(mat, self.k)

    def download_rows(self, mat: torch.Tensor, rows: np.ndarray) -> np.ndarray:
        "rows of a device factor matrix, in the given order, as a host [len(rows) x k] array"
        idx = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(mat.device)
        return self.D.to_host_unpadded(mat.index_select(0, idx), self.k)

    def gramian(self, rows: torch.Tensor, reg: float) -> torch.Tensor:
        return self._gram(rows, reg)

    def half_epoch(self, plan, this_slice, other_full, otor) -> torch.Tensor:
        "-> device scalar sqrt(sum ||delta||^2) of the slice"
        return plan.half_epoch(this_slice, other_full, otor)

    def half_epoch_explicit(self, plan, this_slice, other_full, reg: float) -> torch.Tensor:
        return plan.half_epoch_explicit(this_slice, other_full, reg)

    def check(self, plan):
        plan.check_status()

    def synchronize(self):
        torch.cuda.synchronize(self.dev)


class ImplicitALSEngine:
    "Row-sharded ALS engine; ``explicit=True`` switches to the biased-MF (explicit) model."

    def __init__(
        self,
        ui: sps.csr_array,
        k: int,
        user_reg: float,
        item_reg: float,
        user_init: np.ndarray,
        item_init: np.ndarray,
        backend,
        group=None,
        explicit: bool = False,
        defer_init: bool = False,
        comm=None,
    ):
        self.k = int(k)
        self.backend = backend
        # explicit = the biased-MF model (src/lenskit/als/_explicit.py, explicit.rs): the CSR
        # values are bias-normalised ratings, A = M^T M + reg n I; no Gramian, same exchanges
        self.explicit = bool(explicit)
        self.user_reg, self.item_reg = float(user_reg), float(item_reg)
        self.group = group
        # the collectives: torch.distributed (RCCL) whenever a process group with more than one
        # rank exists -- or a communicator handed in (tests: LoopbackComm)
        force = (os.environ.get("LK_ALS_FORCE_COLLECTIVES", "0") == "1" and dist.is_available()
                 and dist.is_initialized())
        if comm is None and (group is not None or _dist_on() or force):
            comm = TorchComm(group)
        self.comm = comm
        self.world = comm.world if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        # collectives run whenever there is more than one rank; LK_ALS_FORCE_COLLECTIVES=1 makes
        # a single rank with an initialised process group issue them too (the in-place
        # all-gather on the slice view, the k*k + 1 all-reduce, the init broadcast): the way to
        # execute the RCCL path on device tensors on a one-GPU box (tests/test_gpu_rccl.py)
        self.collective = self.world > 1 or force
        n_users, n_items = ui.shape
        self.n_users, self.n_items = n_users, n_items
        on_device = hasattr(ui, "h_indptr")  # a DeviceCSR: the matrix is already in HBM
        if not on_device and hasattr(backend, "make_plans_on_device"):
            # product path: ONE upload of the original CSR; everything derived from it (item
            # counts, relabelling, the other orientation) is computed in HBM
            ui = sps.csr_array(ui)
            ui = backend.D.DeviceCSR.from_arrays(ui.indptr, ui.indices, ui.data, ui.shape,
                                                 backend.dev)
            on_device = True
        if on_device:
            ulen = np.diff(ui.h_indptr)
            ilen = torch.bincount(ui.indices, minlength=n_items).cpu().numpy()
        else:
            ui = sps.csr_array(ui)
            ulen = np.diff(ui.indptr)
            ilen = np.bincount(ui.indices, minlength=n_items)
        # row slices of the overlapped half-epoch (module docstring): only with collectives, and
        # only when a slice is still a full launch
        S = int(os.environ.get("LK_ALS_OVERLAP_SLICES", "0") or 0)
        if not self.collective:
            S = 1
        elif S <= 0:
            # automatic: worth its extra launches (one plan per slice) where the gathered factor
            # matrix is big -- 256 MB and up: cfg5's 10 GB, not cfg2's 41 MB, whose gather is as
            # short as the launches it would add -- and a slice is still a full launch
            gathered = max(n_users, n_items) * getattr(backend, "kp", self.k) * 4
            S = 4 if (gathered >= (256 << 20)
                      and min(n_users, n_items) // self.world >= 4 * 1024) else 1
        self.slices = S
        # strict reference order (LK_ALS_RHS_ORDER=reference on one rank): no relabelling at all
        # (kept from round 4; since round 5 the relabelled engine lists every row's entries in
        # the reference's order too, so this only fixes the ROW order of the launches)
        keep = bool(getattr(backend, "reference_order", False)) and self.world == 1 and S == 1
        def by_length(lens):
            "rows by descending length, ties in row order: on the device when there is one"
            if keep or not on_device or len(lens) < (1 << 16):
                return None
            t = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).to(backend.dev)
            return torch.sort(t, descending=True, stable=True).indices.cpu().numpy()

        self.u_new, self.u_old, self.u_rpr = deal_rows(ulen, self.world, S, keep, by_length(ulen))
        self.i_new, self.i_old, self.i_rpr = deal_rows(ilen, self.world, S, keep, by_length(ilen))
        nu, ni = self.world * self.u_rpr, self.world * self.i_rpr

        r, W = self.rank, self.world
        um, im = self.u_rpr // S, self.i_rpr // S
        # this rank's block of slice s, and the super-block (all ranks' blocks) it lies in
        self.u_blocks = [(s_ * W * um + r * um, s_ * W * um + (r + 1) * um) for s_ in range(S)]
        self.i_blocks = [(s_ * W * im + r * im, s_ * W * im + (r + 1) * im) for s_ in range(S)]
        self.u_supers = [(s_ * W * um, (s_ + 1) * W * um) for s_ in range(S)]
        self.i_supers = [(s_ * W * im, (s_ + 1) * W * im) for s_ in range(S)]
        self.u_lo, self.u_hi = self.u_blocks[0]  # (the whole block of the rank when S == 1)
        self.i_lo, self.i_hi = self.i_blocks[0]
        # LK_ALS_SETUP=sharded (more than one rank): each rank derives only its own rows
        self.sharded_setup = self.world > 1 and sharded_setup()
        if hasattr(backend, "make_plans_on_device"):
            # product path: one upload, relabel + transpose in HBM
            if self.sharded_setup and hasattr(backend, "make_plans_sharded"):
                self.u_plan, self.i_plan, self.local_nnz = backend.make_plans_sharded(
                    ui, self.u_old, self.u_new, self.i_new, ni,
                    self.u_blocks[0] if S == 1 else self.u_blocks,
                    self.i_blocks[0] if S == 1 else self.i_blocks)
            else:
                self.u_plan, self.i_plan, self.local_nnz = backend.make_plans_on_device(
                    ui, self.u_old, self.i_new, self.i_old,
                    self.u_blocks[0] if S == 1 else self.u_blocks,
                    self.i_blocks[0] if S == 1 else self.i_blocks, ilen)
            self.u_plans = [self.u_plan] if S == 1 else self.u_plan.plans
            self.i_plans = [self.i_plan] if S == 1 else self.i_plan.plans
            if hasattr(backend, "order_units"):
                backend.order_units(self.u_plans, self.i_old, self.i_plans, self.u_old)
        elif self.sharded_setup:  # the same per-rank set-up on host tensors (gloo tests)
            assert not on_device
            out = shard_local_blocks(
                torch.from_numpy(ui.indptr.astype(np.int64)),
                torch.from_numpy(ui.indices.astype(np.int32)),
                torch.from_numpy(np.ascontiguousarray(ui.data, dtype=np.float32)),
                self.u_old, self.u_new, self.i_new, self.u_blocks, self.i_blocks,
                by_new_user=True)

            def host_plans(arrs, blocks, n_cols):
                h_ptr, _, idx, val = arrs
                ps, lo = [], 0
                for b_lo, b_hi in blocks:
                    hi = lo + (b_hi - b_lo)
                    a, b = int(h_ptr[lo]), int(h_ptr[hi])
                    ps.append(backend.make_plan(sps.csr_array(
                        (val[a:b].numpy(), idx[a:b].numpy(), h_ptr[lo : hi + 1] - a),
                        shape=(hi - lo, n_cols))))
                    lo = hi
                return ps, int(h_ptr[-1])

            self.u_plans, unnz = host_plans(out["u"], self.u_blocks, ni)
            self.i_plans, innz = host_plans(out["i"], self.i_blocks, nu)
            self.u_plan, self.i_plan = self.u_plans[0], self.i_plans[0]
            self.local_nnz = (unnz, innz)
        else:  # host restatement (CPU / gloo tests of the sharding logic)
            assert not on_device
            ui_new = _relabel_csr(ui, self.u_new, nu, self.i_new, ni)
            iu_new = sps.csr_array(ui_new.T)
            iu_new.sort_indices()
            self.u_plans = [backend.make_plan(ui_new[lo:hi]) for lo, hi in self.u_blocks]
            self.i_plans = [backend.make_plan(iu_new[lo:hi]) for lo, hi in self.i_blocks]
            self.u_plan, self.i_plan = self.u_plans[0], self.i_plans[0]
            self.local_nnz = (
                sum(int(ui_new.indptr[hi] - ui_new.indptr[lo]) for lo, hi in self.u_blocks),
                sum(int(iu_new.indptr[hi] - iu_new.indptr[lo]) for lo, hi in self.i_blocks))

        self._nu, self._ni = nu, ni
        self._qtq = None
        self._ptp = None  # P^T P + item_reg I of the native epoch call (_train_epoch_native)
        # LK_ALS_Z=sharded: the Woodbury operand Z formed once across the ranks.  Whether a half
        # takes it is decided for ALL ranks together (a rank whose own rows need no Z still owes
        # the others its share of the rows): one small all-reduce at set-up
        self._zs = {}
        if (self.world > 1 and not self.explicit and sharded_z() and hasattr(backend, "kp")
                and backend.kp in (128, 256) and hasattr(backend, "D")):
            want = torch.tensor([float(any(getattr(p, "use_wb", False) for p in self.u_plans)),
                                 float(any(getattr(p, "use_wb", False) for p in self.i_plans))],
                                dtype=torch.float32, device=backend.dev)
            self.comm.all_reduce(want)
            want = want.cpu().numpy() > 0
            if want[0]:  # user half: other = Q
                self._zs["u"] = backend.D.ShardedZ(ni, self.k, backend.dev)
            if want[1]:  # item half: other = P
                self._zs["i"] = backend.D.ShardedZ(nu, self.k, backend.dev)
        if not defer_init:
            self.set_initial(user_init, item_init)
        self.epochs_trained = 0

    def set_initial(self, user_init, item_init):
        """
        Initial factors (host arrays in the original labelling, or None for the reference's
        recipe drawn in HBM).  Separate from the constructor so that a trainer can draw the
        host random numbers WHILE the matrix is uploaded, relabelled and transposed.
        """
        backend, nu, ni = self.backend, self._nu, self._ni
        if user_init is None:
            # bench-scale models (10^7 x 256): the reference's recipe ((N(0,1) * 0.01)^2, items
            # first) drawn in HBM instead of crossing PCIe with 11 GB of host random numbers
            self.Q = backend.random_init(ni, self.i_old, seed=1)
            self.P = backend.random_init(nu, self.u_old, seed=2)
        elif hasattr(backend, "upload_permuted"):
            # product path: upload in the original order, permute in HBM
            self.P = backend.upload_permuted(user_init, self.u_new, nu)
            self.Q = backend.upload_permuted(item_init, self.i_new, ni)
        else:
            P = np.zeros((nu, self.k), dtype=np.float32)
            Q = np.zeros((ni, self.k), dtype=np.float32)
            P[self.u_new] = user_init
            Q[self.i_new] = item_init
            self.P = backend.upload(P)
            self.Q = backend.upload(Q)
        if self.collective:
            # every rank must start from the SAME factors (the first user half mixes the local Q
            # with an all-reduced Gramian): rank 0's initialisation wins, whatever the ranks'
            # generators drew (unseeded runs draw differently on every rank)
            self.comm.broadcast(self.P)
            self.comm.broadcast(self.Q)
        # Gramian of the initial Q (user half of epoch 1 needs it); padding rows are 0
        self._qtq = None if self.explicit else self._gramian(self.Q, self.i_blocks,
                                                             self.user_reg)

    # -- collectives ---------------------------------------------------------
    def _own_gramian(self, full: torch.Tensor, blocks, reg: float) -> torch.Tensor:
        "sum of the k x k Gramians of this rank's row blocks (+ reg I once, on rank 0)"
        g = None
        for n_, (lo, hi) in enumerate(blocks):
            part = self.backend.gramian(full[lo:hi], reg if (self.rank == 0 and n_ == 0) else 0.0)
            g = part if g is None else g + part
        return g

    def _gramian(self, full: torch.Tensor, blocks, reg: float) -> torch.Tensor:
        "M^T M + reg I from slice Gramians (k x k all-reduce when sharded)."
        if not self.collective:
            return self.backend.gramian(full, reg)
        g = self._own_gramian(full, blocks, reg)
        self.comm.all_reduce(g)
        return g

    def _half(self, plans, blocks, supers, this: torch.Tensor, other: torch.Tensor, arg):
        """
        One half-epoch, slice by slice: the solve of slice s on the current stream, the in-place
        all-gather of its super-block issued asynchronously right behind it (it runs beside the
        solve of slice s + 1).  Returns (per-slice delta scalars, gather handles to wait on).
        """
        b = self.backend
        ds, handles = [], []
        zs = self._zs.get("u" if plans is self.u_plans else "i") if self._zs else None
        if zs is not None:
            z, flag = zs.form(other, arg, self.rank, self.world, self.comm)
            for plan in plans:
                if plan.use_wb and getattr(plan, "_z_ext", None) is None:
                    plan.set_external_z(z, flag)
        for plan, (lo, hi), (slo, shi) in zip(plans, blocks, supers):
            if self.explicit:
                ds.append(b.half_epoch_explicit(plan, this[lo:hi], other, arg))
            else:
                ds.append(b.half_epoch(plan, this[lo:hi], other, arg))
            if self.collective:
                if len(plans) == 1:
                    self.comm.all_gather_rows(this, lo, hi)
                else:
                    handles.append(self.comm.all_gather_block_async(this, slo, shi, lo, hi))
        return ds, handles

    @staticmethod
    def _wait(handles):
        for h in handles:
            h.wait()

    # -- training ------------------------------------------------------------
    def train_epoch(self):
        "One epoch; returns device tensors (|dP|, |dQ|) -- no host sync inside."
        if self.explicit:
            ds, hs = self._half(self.u_plans, self.u_blocks, self.u_supers, self.P, self.Q,
                                self.user_reg)
            self._wait(hs)
            du = self._delta(ds)
            ds, hs = self._half(self.i_plans, self.i_blocks, self.i_supers, self.Q, self.P,
                                self.item_reg)
            self._wait(hs)
            di = self._delta(ds)
            self.epochs_trained += 1
            return du, di
        if self._native_epoch():
            return self._train_epoch_native()
        # user half: previous Q (src/lenskit/als/_common.py:251)
        ds, hs = self._half(self.u_plans, self.u_blocks, self.u_supers, self.P, self.Q, self._qtq)
        ptp, du = self._gramian_and_delta(self.P, self.u_blocks, self.item_reg, ds, hs)
        # item half: NEW P (_common.py:253)
        ds, hs = self._half(self.i_plans, self.i_blocks, self.i_supers, self.Q, self.P, ptp)
        # Q^T Q + user_reg I: next epoch's user half AND the scorer's _OtOr
        # (_save_user_otor, src/lenskit/als/_implicit.py:171-175)
        self._qtq, di = self._gramian_and_delta(self.Q, self.i_blocks, self.user_reg, ds, hs)
        self.epochs_trained += 1
        return du, di

    def _native_epoch(self) -> bool:
        """
        Does the whole epoch go through ``lk_als_implicit_epoch``?  One device, no collectives,
        one plan per side, and plans the call serves (hybrid order, exact solver, padded k <= 64,
        no task-control block); everything else keeps the per-half calls.
        """
        D = getattr(self.backend, "D", None)
        return (D is not None and hasattr(D, "als_implicit_epoch") and not self.collective
                and not self._zs and len(self.u_plans) == 1 and len(self.i_plans) == 1
                and isinstance(self._qtq, torch.Tensor) and self._qtq.is_cuda
                and D.epoch_plans_ok(self.u_plan, self.i_plan))

    def _train_epoch_native(self):
        b = self.backend
        # the engine's own Gramian is updated in place (nobody else holds it: otor() copies);
        # the deltas are a fresh pair per epoch -- a caller may keep those of several epochs
        qtq = self._qtq
        if self._ptp is None or self._ptp.shape != qtq.shape:
            self._ptp = torch.empty_like(qtq)
        delta = torch.empty(2, dtype=torch.float32, device=qtq.device)
        b.D.als_implicit_epoch(self.u_plan, self.i_plan, self.P, self.Q, qtq, self.user_reg,
                               self._ptp, self.item_reg, b._gram, delta)
        self.epochs_trained += 1
        return delta[0], delta[1]

    def _gramian_and_delta(self, full: torch.Tensor, blocks, reg: float, ds, handles):
        """
        The slice Gramian (k x k) and the slice's squared delta travel in ONE all-reduce
        (k*k + 1 floats: latency-bound on xGMI, so one message instead of two); returns
        (M^T M + reg I, sqrt(sum of squared row deltas)).  The Gramians of the rank's OWN rows are
        formed while the row gathers of the half-epoch are still on the links; the gathers are
        waited for here, before the next half reads the full matrix.
        """
        if not self.collective:
            return self.backend.gramian(full, reg), ds[0].clone()
        g = self._own_gramian(full, blocks, reg)
        kk = self.k * self.k
        buf = torch.empty(kk + 1, dtype=torch.float32, device=g.device)
        buf[:kk] = g.reshape(-1)
        sq = ds[0] * ds[0]
        for d in ds[1:]:
            sq = sq + d * d
        buf[kk:] = sq.reshape(-1)
        self._wait(handles)
        self.comm.all_reduce(buf)
        return buf[:kk].reshape(self.k, self.k).contiguous(), buf[kk:].sqrt()

    def _delta(self, ds) -> torch.Tensor:
        if not self.collective:
            return ds[0].clone()
        sq = ds[0] * ds[0]
        for d in ds[1:]:
            sq = sq + d * d
        self.comm.all_reduce(sq)
        return sq.sqrt()

    def check(self):
        "Synchronise; raise RuntimeError('ALS solve error: ...') if a solve failed."
        for plan in self.u_plans + self.i_plans:
            self.backend.check(plan)

    # -- results (host, original labelling) ------------------------------------
    def user_embeddings(self) -> np.ndarray:
        if hasattr(self.backend, "download_rows"):
            return self.backend.download_rows(self.P, self.u_new)  # gathered in HBM
        return self.backend.download(self.P)[self.u_new]

    def item_embeddings(self) -> np.ndarray:
        if hasattr(self.backend, "download_rows"):
            return self.backend.download_rows(self.Q, self.i_new)
        return self.backend.download(self.Q)[self.i_new]

    def otor(self) -> np.ndarray:
        "Q^T Q + user_reg I (k x k) -- the scorer's ``_OtOr`` (implicit model only)."
        assert not self.explicit
        g = self._qtq
        return g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)


def _global_rank(group, group_rank: int) -> int:
    return dist.get_global_rank(group, group_rank) if group is not None else group_rank


def _dist_on() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
