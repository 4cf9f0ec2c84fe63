"""
Device-side plumbing: torch tensors as HBM buffers, the current torch stream as the
HIP stream, thin typed wrappers over the C ABI (``include/lkamd.h``).

Nothing in here computes: every arithmetic step is a hand-written HIP kernel behind
``lkpy_amd/_lkamd.so``.  PyTorch only owns memory, streams and (elsewhere) the RCCL
process group.
"""

from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from ._native import check


def device(dev=None) -> torch.device:
    _native.require_gpu()
    if dev is None:
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise _native.BackendUnavailable(f"lkpy_amd runs on a HIP device only (got {dev})")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _ptr(t) -> ctypes.c_void_p:
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded_dim(k: int) -> int:
    kp = _native.load().lk_padded_dim(int(k))
    if kp == 0:
        raise ValueError(f"unsupported embedding size {k} (supported: 1..1024)")
    return kp


def to_device_padded(mat: np.ndarray, dev) -> torch.Tensor:
    "Host [n x k] float32 -> device [n x KP] with zero pad columns."
    mat = np.ascontiguousarray(mat, dtype=np.float32)
    n, k = mat.shape
    kp = padded_dim(k)
    src = torch.from_numpy(mat).to(dev)
    if kp == k:
        return src.contiguous()
    dst = torch.empty((n, kp), dtype=torch.float32, device=dev)
    check(_native.load().lk_pad_rows(_ptr(src), n, k, k, _ptr(dst), kp, _stream()), "lk_pad_rows")
    return dst


_NP_OF = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64,
          torch.uint8: np.uint8, torch.float64: np.float64}


def _advise_hugepages(arr: np.ndarray) -> None:
    """
    Ask for transparent huge pages under a freshly allocated destination (``madvise``,
    ``MADV_HUGEPAGE``): a 9.2 GB result is 2.3 M first-touch faults of 4 KiB pages -- host time
    that the download team pays while the link waits -- against 4 600 faults of 2 MiB pages.
    Best effort: silently a no-op where the kernel does not offer it (LK_DOWNLOAD_THP=0: off).
    """
    if os.environ.get("LK_DOWNLOAD_THP", "1") == "0":
        return
    try:
        libc = ctypes.CDLL(None, use_errno=True)
        page = 2 << 20
        beg = (arr.ctypes.data + page - 1) // page * page
        end = (arr.ctypes.data + arr.nbytes) // page * page
        if end > beg:
            libc.madvise(ctypes.c_void_p(beg), ctypes.c_size_t(end - beg), 14)  # MADV_HUGEPAGE
    except Exception:  # noqa: BLE001 -- an optimisation hint only
        pass


def to_host(t: torch.Tensor, threads: int = 0, index_bound: int | None = None) -> np.ndarray:
    """
    A device tensor as a host NumPy array.  Large results (>= 64 MB) go through ``lk_download``
    (pinned staging ring + a team of host threads: PCIe speed into pageable memory instead of
    the ~12 GB/s of a plain copy into fresh pages); small ones are a plain ``.cpu()``.
    ``index_bound``: an int32 tensor whose values are known to lie in [0, index_bound) -- with
    index_bound <= 65 536 it crosses the link as uint16 (``lk_download_i32_narrow``).
    """
    nbytes = t.numel() * t.element_size()
    if t.is_cuda and (256 << 10) <= nbytes < (64 << 20) and t.dtype in _NP_OF:
        # mid-sized results (the [B x n] lists of a batch recommend call: 8 MB): one DMA into a
        # pinned block of torch's caching host allocator -- a plain ``.cpu()`` lands in fresh
        # pageable pages at 10 ... 40 GB/s (0.2 ... 0.8 ms for those 8 MB, measured); the array
        # keeps the block alive and hands it back to the cache when it is dropped
        host = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        return host.numpy()
    if not t.is_cuda or nbytes < (64 << 20) or t.dtype not in _NP_OF:
        return t.cpu().numpy()
    t = t.contiguous()
    out = np.empty(tuple(t.shape), dtype=_NP_OF[t.dtype])
    _advise_hugepages(out)
    lib = _native.require_gpu()
    if (index_bound is not None and index_bound <= 65536 and t.dtype == torch.int32
            and os.environ.get("LK_DOWNLOAD_NARROW", "1") != "0"):
        tmp = torch.empty(t.numel(), dtype=torch.int16, device=t.device)
        check(lib.lk_download_i32_narrow(out.ctypes.data_as(ctypes.c_void_p), _ptr(t), t.numel(),
                                         _ptr(tmp), int(threads), _stream()),
              "lk_download_i32_narrow")
        return out
    check(lib.lk_download(out.ctypes.data_as(ctypes.c_void_p), _ptr(t), nbytes, int(threads),
                          _stream()), "lk_download")
    return out


def to_host_unpadded(mat: torch.Tensor, k: int) -> np.ndarray:
    "Device [n x KP] -> host [n x k] float32."
    n, kp = mat.shape
    if kp == k:
        return mat.cpu().numpy()
    dst = torch.empty((n, k), dtype=torch.float32, device=mat.device)
    check(
        _native.load().lk_unpad_rows(_ptr(mat), n, k, kp, _ptr(dst), k, _stream()),
        "lk_unpad_rows",
    )
    return dst.cpu().numpy()


def lists_to_host(idx: torch.Tensor, scores: torch.Tensor, rows: torch.Tensor | None = None):
    """
    The [B x n] item numbers (int32) and scores (f32) of a batched recommend call as host arrays,
    in one crossing; ``rows`` (device int64 [B]): output row r is input row ``rows[r]``.
    """
    both = torch.cat([idx.view(torch.float32), scores], dim=1)
    host = to_host(both if rows is None else both[rows])
    cols = idx.shape[1]
    return host[:, :cols].view(np.int32), host[:, cols:]


def blank_rows(idx: torch.Tensor, scores: torch.Tensor, valid: np.ndarray) -> None:
    "The rows of a [B x n] top-N result whose query is not ``valid`` (host bool [B]): -1 / NaN."
    if not valid.all():
        bad = torch.from_numpy(np.flatnonzero(~valid)).to(idx.device)
        idx[bad] = -1
        scores[bad] = float("nan")


def blank_panel_rows(panel: torch.Tensor, valid: np.ndarray) -> None:
    "The rows of a [B x items] score panel whose query is not ``valid`` (host bool [B]): NaN."
    if not valid.all():
        panel[torch.from_numpy(np.flatnonzero(~valid)).to(panel.device)] = float("nan")


@dataclass
class DeviceCSR:
    "CSR in HBM: the SparseRowArray layout (offsets i32/i64, indices i32, values f32)."

    indptr: torch.Tensor
    indices: torch.Tensor
    values: torch.Tensor | None  # None: structure only
    shape: tuple[int, int]
    h_indptr: np.ndarray  # host copy of the offsets (plans are built from it)

    @property
    def nnz(self) -> int:
        return int(self.indices.shape[0])

    @property
    def is64(self) -> bool:
        return self.indptr.dtype == torch.int64

    @classmethod
    def from_arrays(cls, indptr, indices, values, shape, dev) -> "DeviceCSR":
        "Host arrays uploaded; ``values=None``: a CSR of structure only (``values`` stays None)."
        indptr = np.ascontiguousarray(indptr)
        if indptr.dtype not in (np.int32, np.int64):
            indptr = indptr.astype(np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float32)
        # zero-copy views of Arrow buffers are read-only; torch.from_numpy wants writable memory
        indptr, indices, values = (a if a is None or a.flags.writeable else a.copy()
                                   for a in (indptr, indices, values))
        return cls(
            torch.from_numpy(indptr).to(dev),
            torch.from_numpy(indices).to(dev),
            None if values is None else torch.from_numpy(values).to(dev),
            (int(shape[0]), int(shape[1])),
            indptr,
        )

    @classmethod
    def from_host(cls, indptr, indices, values, shape, dev) -> "DeviceCSR":
        """
        A model matrix uploaded as the batch scoring calls take it: ``from_arrays`` with the
        offsets int64 whatever the host has (SciPy's are int32).  Nothing is sorted or modified.
        """
        return cls.from_arrays(np.asarray(indptr, dtype=np.int64), indices, values, shape, dev)

    @classmethod
    def from_scipy(cls, mat, dev) -> "DeviceCSR":
        mat = mat.tocsr()
        mat.sort_indices()
        return cls.from_arrays(mat.indptr, mat.indices, mat.data, mat.shape, dev)


class TaskCtl:
    """
    Cancel + progress words of a long-running call (``lk_task_ctl``; the ``AccelTask``
    protocol of src/accel/tasks/mod.rs:62-106): ``cancel()`` may be called from any thread
    while the kernels run, ``progress()`` reads the live row count from pinned host memory.
    """

    def __init__(self):
        lib = _native.require_gpu()
        self._h = ctypes.c_void_p(0)
        check(lib.lk_task_ctl_create(ctypes.byref(self._h)), "lk_task_ctl_create")

    def cancel(self):
        _native.load().lk_task_ctl_cancel(self._h)

    @property
    def cancelled(self) -> bool:
        return bool(_native.load().lk_task_ctl_cancelled(self._h))

    def reset(self):
        _native.load().lk_task_ctl_reset(self._h)

    def progress(self) -> tuple[int, int]:
        "(rows done, rows total) of the call in flight (or of the last finished one)"
        d, t = ctypes.c_int64(0), ctypes.c_int64(0)
        check(_native.load().lk_task_ctl_progress(self._h, ctypes.byref(d), ctypes.byref(t)),
              "lk_task_ctl_progress")
        return int(d.value), int(t.value)

    def __del__(self):
        try:
            if self._h:
                _native.load().lk_task_ctl_destroy(self._h)
                self._h = ctypes.c_void_p(0)
        except Exception:
            pass


class Gramian:
    "``M^T M + reg I`` (lk_gramian) with a reusable workspace."

    def __init__(self, k: int, dev):
        self.k = int(k)
        self.kp = padded_dim(k)
        lib = _native.load()
        self.ws = torch.empty(lib.lk_gramian_workspace_bytes(self.k), dtype=torch.uint8, device=dev)
        self.dev = dev

    def __call__(self, m: torch.Tensor, reg: float, out: torch.Tensor | None = None):
        n, ld = m.shape
        assert ld == self.kp and m.dtype == torch.float32 and m.is_contiguous()
        if out is None:
            out = torch.empty((self.k, self.k), dtype=torch.float32, device=self.dev)
        check(
            _native.load().lk_gramian(
                _ptr(m), n, self.k, ld, float(reg), _ptr(out), out.stride(0), _ptr(self.ws),
                _stream()
            ),
            "lk_gramian",
        )  # fmt: skip
        return out


def als_order_mode(x) -> str:
    "``auto`` / ``reference`` / ``accurate`` from a bool, a string or None (= LK_ALS_RHS_ORDER)"
    if x is None:
        x = os.environ.get("LK_ALS_RHS_ORDER", "") or "auto"
    if x is True:
        return "reference"
    if x is False:
        return "accurate"
    x = str(x).lower()
    if x in ("hybrid", "default"):
        x = "auto"
    if x not in ("auto", "reference", "accurate"):
        raise ValueError(f"unknown LK_ALS_RHS_ORDER {x!r} (auto / reference / accurate)")
    return x


def use_woodbury(kp: int, solver: int, woodbury_rows: int, has_negative) -> bool:
    """
    Do the Woodbury kernels take the short rows of a half-epoch (csrc/als_wb.hip,
    als_wb64_kernel)?  Padded k = 128 / 256, the exact solver, at least ``LK_ALS_WB_MIN_ROWS``
    (default 4096; 0 disables) Woodbury rows -- enough to pay for Z = other @ OtOr^-1 -- and no
    negative confidence value: the kernels take sqrt(v) of every increment, so with negative
    values (use_ratings=True and negative ratings) they would flag rows the dense sposv path
    still solves.  ``has_negative`` is called only when the rest holds (it costs a device scan).
    The library's own host entry (lk_als_implicit_half_epoch_host_ctl) applies the same rule.
    """
    wb_min = int(os.environ.get("LK_ALS_WB_MIN_ROWS", "4096"))
    return (64 < kp <= 256 and solver == _native.SOLVER_CHOLESKY and wb_min > 0
            and woodbury_rows >= wb_min and not has_negative())


class ALSPlan:
    "Row schedule + workspace of one CSR orientation (lk_als_plan)."

    def __init__(self, csr: DeviceCSR, k: int, solver: int = _native.SOLVER_AUTO,
                 reference_order: "bool | str | None" = None, band_units: bool = False):
        """``band_units``: the caller will call :meth:`order_units` (LK_ALS_PLAN_BAND_UNITS: a
        padded k = 64 plan then cuts its long rows into a unit per 256-entry block).

        ``reference_order`` -- how the two long sums of a row (normal matrix, right-hand side)
        are ordered (include/lkamd.h, ``lk_als_plan_create_ex``; INTEGRATION.md, ``LK_ALS_RHS_ORDER``):

        * ``"auto"`` (the default): rows longer than ``LK_ALS_REF_LEN`` (2048) entries in the
          reference's own order (LK_ALS_PLAN_HYBRID_ORDER), the others in the tuned kernels' order;
        * ``"reference"`` / ``True``: strict -- every row of more than 256 entries
          (LK_ALS_PLAN_REFERENCE_ORDER + the rhs workspace);
        * ``"accurate"`` / ``False``: the tuned kernels' own summation on every row (round 4's
          default: closer to the exact solution on rows of 10^4+ entries, up to 7e-2 from the
          reference there);
        * ``None``: what ``LK_ALS_RHS_ORDER`` says (default ``auto``).
        """
        lib = _native.require_gpu()
        self.csr = csr
        self.k = int(k)
        self.kp = padded_dim(k)
        self._h = ctypes.c_void_p(0)
        hp = csr.h_indptr
        self.order_mode = als_order_mode(reference_order)
        if int(solver) == _native.SOLVER_CG or self.kp > 256:
            self.order_mode = "accurate"  # (no reference arithmetic to reproduce / no slab path)
        self.reference_order = self.order_mode == "reference"
        flags = {"accurate": 0, "reference": _native.H["LK_ALS_PLAN_REFERENCE_ORDER"],
                 "auto": _native.H["LK_ALS_PLAN_HYBRID_ORDER"]}[self.order_mode]
        if band_units:
            flags |= _native.H["LK_ALS_PLAN_BAND_UNITS"]
        check(
            lib.lk_als_plan_create_ex(
                ctypes.byref(self._h), hp.ctypes.data_as(ctypes.c_void_p),
                1 if hp.dtype == np.int64 else 0, csr.shape[0], self.k, int(solver), flags
            ),
            "lk_als_plan_create_ex",
        )  # fmt: skip
        dev = csr.indices.device
        self.ws = torch.empty(lib.lk_als_plan_workspace_bytes(self._h), dtype=torch.uint8,
                              device=dev)
        self.frob = torch.zeros(1, dtype=torch.float32, device=dev)
        self.solver = int(lib.lk_als_plan_solver(self._h))
        # rows with <= 64 entries at padded k > 64: Woodbury paths (csrc/als_wb.hip, als_wb64_kernel)
        self.short_rows = int(lib.lk_als_plan_short_rows(self._h))        # <= 16 entries
        # rows the Woodbury kernels take: <= 64 entries at padded k = 256 (<= 128 with the
        # 128 x 128 variant, counted by the caller); at k = 128 <= 16, or <= 32 / 64 with
        # LK_ALS_WB64_K128 (the library applies the same rule)
        self.woodbury_rows = int(lib.lk_als_plan_woodbury_rows(self._h))
        self._negative_values = None  # not scanned yet (one reduction + one host sync)
        self.use_wb = use_woodbury(self.kp, self.solver, self.woodbury_rows,
                                   lambda: self.negative_values)
        self._z = None
        self._z_leader = None  # another slice's plan whose Z this one uses (share_z_from)
        self._z_shared_set = False
        self._yref = None
        if self.reference_order:
            self.set_rhs_order("reference")

    @property
    def negative_values(self) -> bool:
        """
        Does the matrix hold a confidence value below zero?  Scanned on first use and remembered:
        whoever is about to switch the Woodbury kernels on asks -- this plan for itself, an
        ``ALSPlanGroup`` for the half-epoch as a whole (its decision can differ from every
        slice's own: slices each below LK_ALS_WB_MIN_ROWS whose sum is above it).
        """
        if self._negative_values is None:
            v = self.csr.values
            self._negative_values = bool(v is not None and v.numel() > 0 and float(v.min()) < 0.0)
        return self._negative_values

    def set_rhs_order(self, order: str):
        """
        ``"reference"``: every half-epoch forms the right-hand side in the reference's own
        summation order (one sequential float32 chain per feature: implicit.rs:116-117; csrc/
        als_rhs.hip) and the dense kernels solve with it; ``"accurate"`` (default): the solve
        kernels' own slotted / chunked sum.  INTEGRATION.md, ``LK_ALS_RHS_ORDER``.
        """
        if order not in ("reference", "accurate"):
            raise ValueError(f"unknown right-hand-side order {order!r}")
        if order == "accurate" and getattr(self, "reference_order", False):
            raise ValueError("a reference-order plan cannot switch back: build another plan")
        if getattr(self, "order_mode", "accurate") == "auto":
            raise ValueError("a hybrid-order plan owns its right-hand-side buffer: build a plan "
                             "with reference_order='accurate' or 'reference' instead")
        if order == "reference" and self.solver != _native.SOLVER_CHOLESKY:
            return  # the CG option has no reference arithmetic to reproduce
        if order == "reference" and self._yref is None:
            self._yref = torch.zeros((max(self.csr.shape[0], 1), self.kp), dtype=torch.float32,
                                     device=self.csr.indices.device)
        elif order == "accurate":
            self._yref = None
        check(_native.load().lk_als_plan_set_rhs_workspace(
            self._h, _ptr(self._yref) if self._yref is not None else None),
            "lk_als_plan_set_rhs_workspace")

    def long_rows(self) -> int:
        "rows of the plan that are pre-reduced in chunks (the first tasks of the longest-first order)"
        return int(_native.load().lk_als_plan_long_rows(self._h))

    def order_units(self, col_key: "torch.Tensor | None" = None):
        """
        Once at set-up (it blocks): list the long rows' work units band by band per XCD instead of
        row by row (``lk_als_plan_order_units``).  ``col_key``: int32 device map
        under which the rows' entries ascend (original-of-new for a relabelled matrix); None =
        the columns themselves.  No result changes; ``LK_ALS_UNIT_ORDER=0`` keeps today's order.
        """
        if col_key is not None:
            assert col_key.dtype == torch.int32 and col_key.is_contiguous()
        check(_native.load().lk_als_plan_order_units(
            self._h, _ptr(self.csr.indices), _ptr(col_key) if col_key is not None else None,
            0 if col_key is None else col_key.numel(), _stream()), "lk_als_plan_order_units")

    def unit_table(self):
        "(first entry, entries, first slab) of the work units in launch order, as host arrays"
        lib = _native.load()
        n = int(lib.lk_als_plan_units(self._h))
        beg, ln, slab = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        check(lib.lk_als_plan_unit_table(self._h, as_p(beg), as_p(ln), as_p(slab)),
              "lk_als_plan_unit_table")
        return beg, ln, slab

    def yref_tasks(self) -> "torch.Tensor | None":
        """Hybrid plans: the right-hand sides the last half-epoch formed in the reference's order,
        [long_rows x KP], row t = the t-th longest row (a view of the workspace); else None."""
        lib = _native.load()
        ptr = lib.lk_als_plan_yref(self._h, _ptr(self.ws))
        if not ptr:
            return None
        off = int(ptr) - int(self.ws.data_ptr())
        n = self.long_rows() * self.kp
        return self.ws[off : off + 4 * n].view(torch.float32).view(-1, self.kp)

    def share_z_from(self, leader: "ALSPlan"):
        """
        Row slices of one half-epoch share one Z = other @ OtOr^-1: ``leader`` (launched first in
        every half-epoch) owns the buffer and forms Z, this plan reads it and copies the leader's
        "OtOr is not positive definite" flag at every launch (lk_als_plan_set_z_shared).
        """
        self._z_leader = leader
        check(_native.load().lk_als_plan_set_z_leader(leader._h, 1), "lk_als_plan_set_z_leader")

    def set_external_z(self, z: torch.Tensor, flag: torch.Tensor):
        """
        Z = other @ OtOr^-1 formed OUTSIDE the plan for every half-epoch (:class:`ShardedZ`: each
        rank forms its share of the rows, one all-gather; ``LK_ALS_Z=sharded``): the plan reads
        ``z`` and copies ``flag`` ("OtOr is not positive definite") into its status word at every
        launch (lk_als_plan_set_z_shared) instead of running the n_cols x KP x KP GEMM itself.
        """
        assert z.shape[1] == self.kp and z.shape[0] == self.csr.shape[1] and z.is_contiguous()
        self._z_ext = (z, flag)  # kept alive with the plan
        check(_native.load().lk_als_plan_set_z_shared(self._h, _ptr(z), _ptr(flag)),
              "lk_als_plan_set_z_shared")
        self._z_shared_set = True

    def set_ctl(self, ctl: "TaskCtl | None"):
        "Attach (or detach) a cancel / progress block; check_status then reports a cancel."
        self._ctl = ctl  # keep it alive as long as the plan refers to it
        check(_native.load().lk_als_plan_set_ctl(self._h, ctl._h if ctl is not None else None),
              "lk_als_plan_set_ctl")

    def set_cg(self, tol: float, max_iter: int = 0):
        check(_native.load().lk_als_plan_set_cg(self._h, float(tol), int(max_iter)),
              "lk_als_plan_set_cg")

    def cg_stats(self):
        "(CG iterations, non-empty rows) of the last CG half-epoch on this plan (blocking)"
        import ctypes

        it, rows = ctypes.c_int64(0), ctypes.c_int64(0)
        check(_native.load().lk_als_plan_cg_stats(self._h, _ptr(self.ws), _stream(),
                                                   ctypes.byref(it), ctypes.byref(rows)),
              "lk_als_plan_cg_stats")
        return int(it.value), int(rows.value)

    def half_epoch(self, this: torch.Tensor, other: torch.Tensor, otor: torch.Tensor):
        """
        One ALS half-epoch on the current stream; ``this`` ([rows x KP]) is updated in
        place.  Asynchronous: returns the device scalar holding sqrt(sum ||delta||^2).
        """
        csr = self.csr
        assert this.shape == (csr.shape[0], self.kp) and other.shape == (csr.shape[1], self.kp)
        assert this.is_contiguous() and other.is_contiguous() and otor.is_contiguous()
        if self.use_wb and getattr(self, "_z_ext", None) is not None:
            pass  # Z arrives from outside (set_external_z)
        elif self.use_wb and self._z_leader is not None:
            if not self._z_shared_set:
                ld = self._z_leader
                assert ld._z is not None, "the leading slice's half-epoch must be launched first"
                lib = _native.load()
                check(lib.lk_als_plan_set_z_shared(self._h, _ptr(ld._z),
                                                   lib.lk_als_plan_z_flag(ld._h, _ptr(ld.ws))),
                      "lk_als_plan_set_z_shared")
                self._z_shared_set = True
        elif self.use_wb and self._z is None:
            # the library forms Z = other @ OtOr^-1 itself at every half-epoch (OtOr^-1 to float64
            # accuracy on the device, csrc/spd_inverse.hip; Z on the scoring GEMM): this side only
            # lends it the [n_cols x KP] buffer -- no library factorisation, no host round trip
            self._z = torch.empty((csr.shape[1], self.kp), dtype=torch.float32,
                                  device=other.device)
            check(_native.load().lk_als_plan_set_z_workspace(self._h, _ptr(self._z)),
                  "lk_als_plan_set_z_workspace")
        check(
            _native.load().lk_als_implicit_half_epoch(
                self._h, _ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values),
                csr.shape[0], csr.shape[1], self.k, _ptr(this), self.kp, _ptr(other), self.kp,
                _ptr(otor), otor.stride(0), _ptr(self.ws), _ptr(self.frob), _stream()
            ),
            "lk_als_implicit_half_epoch",
        )  # fmt: skip
        return self.frob

    def half_epoch_explicit(self, this: torch.Tensor, other: torch.Tensor, reg: float):
        """
        One explicit-feedback (biased-MF) half-epoch (lk_als_explicit_half_epoch;
        src/accel/als/explicit.rs:33-119): the CSR values are the bias-normalised ratings.
        """
        csr = self.csr
        assert this.shape == (csr.shape[0], self.kp) and other.shape == (csr.shape[1], self.kp)
        assert this.is_contiguous() and other.is_contiguous()
        check(
            _native.load().lk_als_explicit_half_epoch(
                self._h, _ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values),
                csr.shape[0], csr.shape[1], self.k, _ptr(this), self.kp, _ptr(other), self.kp,
                float(np.float32(reg)), _ptr(self.ws), _ptr(self.frob), _stream()
            ),
            "lk_als_explicit_half_epoch",
        )  # fmt: skip
        return self.frob

    def enable_timing(self, enable: bool = True):
        check(_native.load().lk_als_plan_enable_timing(self._h, 1 if enable else 0),
              "lk_als_plan_enable_timing")

    def get_timing(self):
        "-> (ms in the chunk kernel, ms in the solve kernel, half-epochs recorded); resets."
        a, b, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int32(0)
        check(
            _native.load().lk_als_plan_get_timing(
                self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)
            ),
            "lk_als_plan_get_timing",
        )
        return a.value, b.value, n.value

    def check_status(self):
        "Synchronise and raise RuntimeError('ALS solve error: ...') on a failed solve."
        check(_native.load().lk_als_check_status(self._h, _ptr(self.ws), _stream()),
              "lk_als_check_status")

    def __del__(self):
        try:
            if self._h:
                _native.load().lk_als_plan_destroy(self._h)
                self._h = ctypes.c_void_p(0)
        except Exception:
            pass


def epoch_plans_ok(u_plan, i_plan) -> bool:
    "Can ``lk_als_implicit_epoch`` run these two plans (include/lkamd.h)?  Else: the half-epoch calls."
    return all(
        isinstance(p, ALSPlan) and p.order_mode == "auto" and p.kp <= 64
        and p.solver == _native.SOLVER_CHOLESKY and getattr(p, "_ctl", None) is None
        for p in (u_plan, i_plan)
    ) and u_plan is not i_plan and u_plan.k == i_plan.k


def als_implicit_epoch(u_plan: "ALSPlan", i_plan: "ALSPlan", P: torch.Tensor, Q: torch.Tensor,
                       qtq: torch.Tensor, user_reg: float, ptp: torch.Tensor, item_reg: float,
                       gram: Gramian, out_delta: torch.Tensor):
    """
    One implicit epoch on the current stream (lk_als_implicit_epoch): ``P`` and ``Q`` updated in
    place, ``qtq`` (Q^T Q + user_reg I) in and out, ``ptp`` out, ``out_delta`` = (|dP|, |dQ|).
    Asynchronous; everything is ordered on the current stream when it returns.
    """
    uc, ic = u_plan.csr, i_plan.csr
    kp = u_plan.kp
    assert P.shape == (uc.shape[0], kp) and Q.shape == (ic.shape[0], kp)
    assert uc.shape[1] == ic.shape[0] and ic.shape[1] == uc.shape[0]
    assert P.is_contiguous() and Q.is_contiguous() and qtq.is_contiguous() and ptp.is_contiguous()
    assert qtq.shape == (u_plan.k, u_plan.k) == ptp.shape and gram.k == u_plan.k
    assert out_delta.numel() == 2 and out_delta.dtype == torch.float32
    check(
        _native.load().lk_als_implicit_epoch(
            u_plan._h, i_plan._h, _ptr(uc.indptr), _ptr(uc.indices), _ptr(uc.values),
            _ptr(ic.indptr), _ptr(ic.indices), _ptr(ic.values), u_plan.k, _ptr(P), _ptr(Q),
            _ptr(qtq), qtq.stride(0), float(user_reg), _ptr(ptp), ptp.stride(0), float(item_reg),
            _ptr(u_plan.ws), _ptr(i_plan.ws), _ptr(gram.ws), _ptr(out_delta), _stream()
        ),
        "lk_als_implicit_epoch",
    )  # fmt: skip


class ShardedZ:
    """
    Z = other @ OtOr^-1 (the Woodbury kernels' operand at padded k = 128 / 256) formed ONCE ACROSS
    THE RANKS instead of once per rank: every rank inverts the k x k OtOr (spd_inverse.hip,
    microseconds), multiplies its own 1 / world share of the rows of ``other`` (the scoring GEMM)
    and the shares are all-gathered in place.  With the default (``LK_ALS_Z=replicated``) every
    rank runs the whole n_cols x KP x KP GEMM -- work that does not shrink with the number of
    GPUs (the cap on cfg5's scaling); sharded it costs one more all-gather of
    the size of the factor gather.  Same bits either way: a row of Z depends on that row of
    ``other`` and on OtOr^-1 only.
    """

    def __init__(self, n_rows: int, k: int, dev):
        lib = _native.require_gpu()
        self.k, self.kp = int(k), padded_dim(k)
        assert self.kp in (128, 256)
        self.z = torch.empty((n_rows, self.kp), dtype=torch.float32, device=dev)
        self.ginv = torch.empty((self.kp, self.kp), dtype=torch.float32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(lib.lk_spd_inverse_workspace_bytes(self.k), dtype=torch.uint8,
                              device=dev)

    def form(self, other: torch.Tensor, otor: torch.Tensor, rank: int, world: int, comm):
        lib = _native.load()
        n = other.shape[0]
        assert n == self.z.shape[0] and n % world == 0 and other.is_contiguous()
        self.flag.zero_()
        check(lib.lk_spd_inverse(_ptr(otor), otor.stride(0), self.k, _ptr(self.ginv),
                                 _ptr(self.flag), _ptr(self.ws), _stream()), "lk_spd_inverse")
        share = n // world
        lo, hi = rank * share, (rank + 1) * share
        if share:
            check(lib.lk_score_dense(_ptr(other[lo:hi]), self.kp, share, _ptr(self.ginv), self.kp,
                                     self.kp, self.k, _ptr(self.z[lo:hi]), self.kp, _stream()),
                  "lk_score_dense")
            comm.all_gather_rows(self.z, lo, hi)
        return self.z, self.flag


class ALSPlanGroup:
    """
    The plans of the ROW SLICES of one orientation on one rank (the sharded engine cuts a rank's
    rows into slices so that the all-gather of one slice runs under the solve of the next),
    presented as one plan to whoever only asks about it (bench / tests): timing and statistics
    are summed, settings go to every slice.  The slices share one Z (the first slice leads).
    """

    def __init__(self, plans: list[ALSPlan], n_cols: int):
        from types import SimpleNamespace

        assert len(plans) >= 1
        self.plans = plans
        p0 = plans[0]
        self.k, self.kp, self.solver = p0.k, p0.kp, p0.solver
        lens = np.concatenate([np.diff(p.csr.h_indptr) for p in plans])
        h = np.zeros(len(lens) + 1, dtype=p0.csr.h_indptr.dtype)
        np.cumsum(lens, out=h[1:])
        # the rank's rows in slice order (row lengths / shapes only: the slices are not contiguous)
        self.csr = SimpleNamespace(h_indptr=h, indices=p0.csr.indices, values=p0.csr.values,
                                   shape=(len(lens), n_cols),
                                   full_h_indptr=getattr(p0.csr, "full_h_indptr", None))
        self.short_rows = sum(p.short_rows for p in plans)
        self.woodbury_rows = sum(p.woodbury_rows for p in plans)

        def has_negative() -> bool:
            # the slices are views into ONE values array (offsets are not rebased): scan each
            # distinct array once, whether or not a slice had reason to look on its own
            seen = {}
            for p in plans:
                v = p.csr.values
                key = None if v is None else (v.data_ptr(), v.numel())
                if key not in seen:
                    seen[key] = p.negative_values
                else:
                    p._negative_values = seen[key]
            return any(seen.values())

        # the Woodbury decision belongs to the half-epoch, not to a slice of it
        use_wb = use_woodbury(self.kp, self.solver, self.woodbury_rows, has_negative)
        for p in plans:
            p.use_wb = use_wb
        for p in plans[1:]:
            p.share_z_from(p0)

    @property
    def use_wb(self) -> bool:
        return bool(self.plans[0].use_wb)

    def set_cg(self, tol: float, max_iter: int = 0):
        for p in self.plans:
            p.set_cg(tol, max_iter)

    def set_rhs_order(self, order: str):
        for p in self.plans:
            p.set_rhs_order(order)

    def cg_stats(self):
        st = [p.cg_stats() for p in self.plans]
        return sum(s[0] for s in st), sum(s[1] for s in st)

    def set_ctl(self, ctl):
        for p in self.plans:
            p.set_ctl(ctl)

    def enable_timing(self, enable: bool = True):
        for p in self.plans:
            p.enable_timing(enable)

    def get_timing(self):
        "-> (chunk ms, solve ms summed over the slices, half-epochs recorded)"
        ts = [p.get_timing() for p in self.plans]
        return sum(t[0] for t in ts), sum(t[1] for t in ts), ts[0][2]

    def check_status(self):
        for p in self.plans:
            p.check_status()


def iknn_build(ui: DeviceCSR, iu: DeviceCSR, min_sim: float, save_nbrs=None,
               rows: tuple[int, int] | None = None, ctl: "TaskCtl | None" = None,
               timing: dict | None = None) -> DeviceCSR:
    """
    Item-item similarity build (lk_iknn_build_count / _fill, then lk_iknn_truncate_* when
    ``save_nbrs`` is set): ``ui`` users x items and ``iu`` items x users hold the normalised
    ratings; returns the similarity matrix as a device CSR with int64 offsets, rows sorted
    by column.  ``rows = (begin, end)`` builds only that block of output rows (one rank's
    shard: rows are independent, no collective); the result then has ``end - begin`` rows.
    """
    lib = _native.require_gpu()
    n_users, n_items = ui.shape
    r0, r1 = (0, n_items) if rows is None else (int(rows[0]), int(rows[1]))
    n_rows = r1 - r0
    assert iu.shape == (n_items, n_users)
    assert ui.h_indptr.dtype == iu.h_indptr.dtype
    dev = ui.indices.device
    is64 = 1 if ui.h_indptr.dtype == np.int64 else 0
    h = ctypes.c_void_p(0)
    check(
        lib.lk_iknn_plan_create_rows(
            ctypes.byref(h), ui.h_indptr.ctypes.data_as(ctypes.c_void_p),
            iu.h_indptr.ctypes.data_as(ctypes.c_void_p), is64, n_users, n_items, r0, r1
        ),
        "lk_iknn_plan_create_rows",
    )  # fmt: skip
    try:
        if ctl is not None:
            check(lib.lk_iknn_plan_set_ctl(h, ctl._h), "lk_iknn_plan_set_ctl")
        if timing is not None:
            check(lib.lk_iknn_plan_enable_timing(h, 1), "lk_iknn_plan_enable_timing")
        ws = torch.empty(lib.lk_iknn_plan_workspace_bytes(h), dtype=torch.uint8, device=dev)
        out_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        total = ctypes.c_int64(0)
        ms = float(np.float32(min_sim))  # cast to f32 at the boundary (item_train.rs:37)
        check(
            lib.lk_iknn_build_count(
                h, _ptr(ui.indptr), _ptr(ui.indices), _ptr(ui.values), _ptr(iu.indptr),
                _ptr(iu.indices), _ptr(iu.values), ms, -1, _ptr(ws), _ptr(out_ptr),
                ctypes.byref(total), _stream()
            ),
            "lk_iknn_build_count",
        )  # fmt: skip
        nnz = int(total.value)
        out_idx = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        out_val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)[:nnz]
        check(
            lib.lk_iknn_build_fill(
                h, _ptr(ui.indptr), _ptr(ui.indices), _ptr(ui.values), _ptr(iu.indptr),
                _ptr(iu.indices), _ptr(iu.values), ms, -1, _ptr(ws), _ptr(out_ptr),
                _ptr(out_idx), _ptr(out_val), _stream()
            ),
            "lk_iknn_build_fill",
        )  # fmt: skip
        torch.cuda.current_stream().synchronize()
        if timing is not None:
            ms, nl = ctypes.c_double(0), ctypes.c_int32(0)
            check(lib.lk_iknn_plan_get_timing(h, ctypes.byref(ms), ctypes.byref(nl)),
                  "lk_iknn_plan_get_timing")
            timing["build_kernel_ms"] = ms.value
            timing["build_kernel_launches"] = nl.value
    finally:
        lib.lk_iknn_plan_destroy(h)
    full = DeviceCSR(out_ptr, out_idx, out_val, (n_rows, n_items), None)
    if save_nbrs is None or int(save_nbrs) <= 0:
        return full
    # item_train.rs:139-151: per-row top-save_nbrs, ties in order of first encounter
    del ws
    tws = torch.empty(lib.lk_iknn_truncate_workspace_bytes(n_rows, nnz), dtype=torch.uint8,
                      device=dev)
    new_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    check(
        lib.lk_iknn_truncate_count(
            _ptr(full.indptr), _ptr(full.indices), _ptr(full.values), _ptr(iu.indptr), is64,
            _ptr(iu.indices), n_rows, r0, nnz, int(save_nbrs), _ptr(tws), _ptr(new_ptr),
            ctypes.byref(total), _stream()
        ),
        "lk_iknn_truncate_count",
    )  # fmt: skip
    nnz2 = int(total.value)
    t_idx = torch.empty(max(nnz2, 1), dtype=torch.int32, device=dev)[:nnz2]
    t_val = torch.empty(max(nnz2, 1), dtype=torch.float32, device=dev)[:nnz2]
    check(
        lib.lk_iknn_truncate_fill(
            _ptr(full.indptr), _ptr(full.indices), _ptr(full.values), n_rows, nnz, _ptr(tws),
            _ptr(new_ptr), _ptr(t_idx), _ptr(t_val), _stream()
        ),
        "lk_iknn_truncate_fill",
    )  # fmt: skip
    torch.cuda.current_stream().synchronize()
    return DeviceCSR(new_ptr, t_idx, t_val, (n_rows, n_items), None)


def score_topk(users: torch.Tensor, items: torch.Tensor, k: int, n: int,
               excl_ptr: torch.Tensor | None = None, excl_items: torch.Tensor | None = None):
    """
    Batched dense scoring + top-N (lk_score_topk): ``users`` [B x KP], ``items`` [I x KP]
    padded device matrices; exclusion CSR (int64 offsets, int32 items) optional.
    Returns (indices int32 [B x n] with -1 padding, scores f32 [B x n] with NaN padding).
    """
    lib = _native.require_gpu()
    B, kp = users.shape
    I = items.shape[0]
    assert kp == padded_dim(k) and items.shape[1] == kp
    assert users.is_contiguous() and items.is_contiguous()
    dev = users.device
    n = int(n)
    cols = I if n < 0 else n  # n < 0: rank every candidate (TopNRanker without n)
    ws = torch.empty(lib.lk_score_topk_workspace_bytes(B, I, n), dtype=torch.uint8, device=dev)
    out_idx = torch.empty((B, cols), dtype=torch.int32, device=dev)
    out_sc = torch.empty((B, cols), dtype=torch.float32, device=dev)
    if excl_ptr is not None:
        assert excl_ptr.dtype == torch.int64 and excl_items.dtype == torch.int32
    check(
        lib.lk_score_topk(
            _ptr(users), kp, B, _ptr(items), kp, I, int(k), int(n), _ptr(excl_ptr),
            _ptr(excl_items), _ptr(ws), _ptr(out_idx), _ptr(out_sc), _stream()
        ),
        "lk_score_topk",
    )  # fmt: skip
    return out_idx, out_sc


def score_topk_last_report() -> dict:
    """
    What this thread's last ``score_topk`` call did (lk_score_topk_last_report; test hook, not for
    product code): path, fused geometry, and the rows redone exactly through the panel path.
    """
    import ctypes

    out = (ctypes.c_int64 * 12)()
    rows = (ctypes.c_int32 * 4096)()
    m = _native.load().lk_score_topk_last_report(out, rows, 4096)
    names = ("path", "batches", "parts", "part_cap", "overlap", "n_redo", "all_panel", "stride",
             "n_sample", "r_tau", "kp", "cmax")
    rep = {k: int(v) for k, v in zip(names, out)}
    rep["path"] = {1: "fused", 0: "panel"}.get(rep["path"])
    rep["overlap"], rep["all_panel"], rep["cmax"] = (bool(rep[k]) for k in ("overlap", "all_panel", "cmax"))
    rep["redo_rows"] = sorted(int(rows[i]) for i in range(m))
    return rep


def argtopn(scores: torch.Tensor, n: int) -> torch.Tensor:
    """
    Per-row top-N indices (lk_argtopn) of a [rows x len] f32 device matrix, -1 padding;
    ``n < 0`` ranks every valid entry (``argsort_descending``).  Lists of up to 4096 take the
    selection kernel, longer ones (and ``n < 0``) the full stable sort.
    """
    lib = _native.require_gpu()
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 2
    rows, ln = scores.shape
    n = int(n)
    cols = ln if n < 0 else min(n, ln)
    out = torch.empty((rows, cols), dtype=torch.int32, device=scores.device)
    if cols == 0 or rows == 0:
        return out
    wb = lib.lk_argtopn_workspace_bytes(rows, ln, n if n < 0 else cols)
    ws = torch.empty(wb, dtype=torch.uint8, device=scores.device) if wb else None
    check(lib.lk_argtopn(_ptr(scores), rows, ln, n if n < 0 else cols, _ptr(ws), _ptr(out),
                         _stream()), "lk_argtopn")
    return out


def iknn_score_batch(sims: DeviceCSR, ref_ptr, ref_items, ref_rates, tgt_ptr, tgt_items,
                     max_nbrs: int, min_nbrs: int):
    """
    Item-kNN scoring of a batch of queries (lk_iknn_score_batch).  ``sims``: similarity CSR
    (int64 offsets); ``ref_*``/``tgt_*``: CSR-style (int64 offsets, int32 items) history and
    target lists, negative items are nulls; ``ref_rates`` f32 (explicit) or None (implicit).
    Returns (scores f32 with NaN for null, counts int32 with -1 for null targets).
    """
    lib = _native.require_gpu()
    n_items = sims.shape[0]
    nq = int(ref_ptr.shape[0]) - 1
    dev = sims.indices.device
    assert sims.indptr.dtype == torch.int64
    if int(tgt_items.shape[0]) == 0:  # (empty target lists only: an empty tensor has no address)
        return (torch.empty(0, dtype=torch.float32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    ws = torch.empty(lib.lk_iknn_score_workspace_bytes(n_items, nq, int(max_nbrs)),
                     dtype=torch.uint8, device=dev)
    out_s = torch.empty(int(tgt_items.shape[0]), dtype=torch.float32, device=dev)
    out_c = torch.empty(int(tgt_items.shape[0]), dtype=torch.int32, device=dev)
    check(
        lib.lk_iknn_score_batch(
            _ptr(sims.indptr), _ptr(sims.indices), _ptr(sims.values), n_items, nq,
            _ptr(ref_ptr), _ptr(ref_items), _ptr(ref_rates), _ptr(tgt_ptr), _ptr(tgt_items),
            int(max_nbrs), int(min_nbrs), _ptr(ws), _ptr(out_s), _ptr(out_c), _stream()
        ),
        "lk_iknn_score_batch",
    )  # fmt: skip
    return out_s, out_c


def bias_user_offsets(hist: DeviceCSR, user_nums: torch.Tensor, global_bias: float,
                      item_biases: torch.Tensor | None, damping_user: float):
    """
    User biases of a batch of queries from their training ratings (lk_bias_user_offsets):
    ``BiasModel.compute_for_items`` with the query's history (src/lenskit/basic/bias.py:166-240)
    for every query at once, bit for bit.  ``hist``: the training matrix in HBM (users x items,
    f32 ratings); ``user_nums``: device int32 [B], -1 = no training row; ``item_biases``: device
    f32 [n_items] or None.  Returns device (ub f32 [B], add uint8 [B]: 1 where the host would add
    ub, i.e. the query has a training row).
    """
    lib = _native.require_gpu()
    dev = hist.indices.device
    B = int(user_nums.shape[0])
    ub = torch.empty(B, dtype=torch.float32, device=dev)
    add = torch.empty(B, dtype=torch.uint8, device=dev)
    assert user_nums.dtype == torch.int32 and hist.values is not None
    check(
        lib.lk_bias_user_offsets(
            _ptr(hist.indptr), 1 if hist.is64 else 0, _ptr(hist.indices), _ptr(hist.values),
            hist.shape[0], hist.shape[1], B, _ptr(user_nums), float(global_bias),
            _ptr(item_biases), float(damping_user), _ptr(ub), _ptr(add), _stream()
        ),
        "lk_bias_user_offsets",
    )  # fmt: skip
    return ub, add


def bias_fit(csr: DeviceCSR, csr_t: DeviceCSR | None, global_bias: float, damping_item: float,
             damping_user: float, *, items: bool = True, users: bool = True):
    """
    ``BiasModel.learn`` on the device (lk_bias_fit_pass, src/lenskit/basic/bias.py:83-150):
    ``csr`` the ratings (users x items, f32 values, entries in dataset order), ``csr_t`` its stable
    transpose with values (:func:`csr_transpose`; needed for the item pass only).  Returns device
    f32 (item biases | None, user biases | None) -- the host's bits: per bin two float64 chains
    in dataset order, the user pass over the ratings less the item biases.
    """
    lib = _native.require_gpu()
    dev = csr.indices.device
    n_users, n_items = csr.shape
    assert csr.values is not None and csr.values.dtype == torch.float32
    ib = ub = None
    if items:
        assert csr_t is not None and csr_t.values is not None and csr_t.shape == (n_items, n_users)
        ib = torch.zeros(n_items, dtype=torch.float32, device=dev)
        check(
            lib.lk_bias_fit_pass(_ptr(csr_t.indptr), 1 if csr_t.is64 else 0, _ptr(None),
                                 _ptr(csr_t.values), n_items, float(global_bias), _ptr(None), 0,
                                 float(damping_item), _ptr(ib), _stream()),
            "lk_bias_fit_pass",
        )
    if users:
        ub = torch.zeros(n_users, dtype=torch.float32, device=dev)
        check(
            lib.lk_bias_fit_pass(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                                 _ptr(csr.values), n_users, float(global_bias), _ptr(ib), n_items,
                                 float(damping_user), _ptr(ub), _stream()),
            "lk_bias_fit_pass",
        )
    return ib, ub


def bias_score_panel(n_items: int, global_bias: float, item_biases: torch.Tensor | None,
                     user_bias: torch.Tensor, user_add: torch.Tensor, *,
                     strike: DeviceCSR | None = None, user_nums: torch.Tensor | None = None):
    """
    The [B x n_items] f32 panel of ``BiasScorer`` scores (lk_bias_score_panel): cell (q, i) =
    (float32(mu) + b_i) + ub_q, the user term where ``user_add[q]``; with ``strike`` (the training
    matrix) and ``user_nums`` (device int32 [B]) NaN at each query's own training items.
    """
    lib = _native.require_gpu()
    B = int(user_bias.shape[0])
    panel = torch.empty((B, int(n_items)), dtype=torch.float32, device=user_bias.device)
    assert user_add.dtype == torch.uint8 and (user_nums is None or user_nums.dtype == torch.int32)
    check(
        lib.lk_bias_score_panel(
            B, int(n_items), float(global_bias), _ptr(item_biases), _ptr(user_bias),
            _ptr(user_add), _ptr(panel), int(n_items),
            _ptr(strike.indptr if strike is not None else None),
            1 if strike is not None and strike.is64 else 0,
            _ptr(strike.indices if strike is not None else None),
            strike.shape[0] if strike is not None else 0,
            _ptr(user_nums if strike is not None else None), _stream()
        ),
        "lk_bias_score_panel",
    )  # fmt: skip
    return panel


def bias_score_ragged(tgt_ptr: torch.Tensor, tgt_items: torch.Tensor, n_items: int,
                      global_bias: float, item_biases: torch.Tensor | None,
                      user_bias: torch.Tensor, user_add: torch.Tensor):
    """
    ``BiasScorer`` scores at ragged targets (lk_bias_score_ragged): device f32 [entries], entry t
    of query q is (float32(mu) + b_item) + ub_q; an unknown item (negative) has no item term and
    is not NaN.  ``tgt_ptr`` device int64 [B + 1], ``tgt_items`` device int32.
    """
    lib = _native.require_gpu()
    n = int(tgt_items.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=tgt_items.device)
    assert tgt_ptr.dtype == torch.int64 and tgt_items.dtype == torch.int32
    check(
        lib.lk_bias_score_ragged(int(tgt_ptr.shape[0]) - 1, _ptr(tgt_ptr), _ptr(tgt_items), n,
                                 int(n_items), float(global_bias), _ptr(item_biases),
                                 _ptr(user_bias), _ptr(user_add), _ptr(out), _stream()),
        "lk_bias_score_ragged",
    )
    return out


def predict_merge(tgt_ptr: torch.Tensor, tgt_items: torch.Tensor, n_items: int,
                  scores: torch.Tensor, item_means: torch.Tensor | None, *,
                  fallback: bool = False, global_bias: float = 0.0,
                  item_biases: torch.Tensor | None = None, user_bias: torch.Tensor | None = None,
                  user_add: torch.Tensor | None = None, out_is_fallback: torch.Tensor | None = None):
    """
    The rating-predictor tail for a batch (lk_predict_merge), in place on ``scores`` (the
    :func:`iknn_score_batch` output over ``tgt_ptr`` / ``tgt_items``): the item means added back
    (item.py:282), and with ``fallback`` the NaN scores replaced by the ``BiasScorer`` score
    mu + b_i (+ ``user_bias`` where ``user_add``) as ``FallbackScorer`` does
    (basic/composite.py).  ``out_is_fallback``: device uint8 [entries] or None.
    """
    lib = _native.require_gpu()
    n = int(tgt_items.shape[0])
    assert scores.dtype == torch.float32 and int(scores.shape[0]) == n
    assert tgt_ptr.dtype == torch.int64 and tgt_items.dtype == torch.int32
    assert out_is_fallback is None or (out_is_fallback.dtype == torch.uint8
                                       and int(out_is_fallback.shape[0]) >= n)
    check(
        lib.lk_predict_merge(
            int(tgt_ptr.shape[0]) - 1, _ptr(tgt_ptr), _ptr(tgt_items), n, int(n_items),
            _ptr(scores), _ptr(item_means), 1 if fallback else 0, float(global_bias),
            _ptr(item_biases), _ptr(user_bias), _ptr(user_add), _ptr(out_is_fallback), _stream()
        ),
        "lk_predict_merge",
    )  # fmt: skip
    return scores


def bmf_residual_rows(mat: DeviceCSR, rows: np.ndarray, global_bias: float,
                      item_biases: torch.Tensor, damping_user: float):
    """
    The fold-in input of ``BiasedMFScorer`` for a batch of training histories
    (lk_bmf_residual_rows): the rows ``rows`` (HOST int32, -1 = an empty row) of the training
    matrix ``mat`` (users x items, f32 ratings, item-sorted rows) with the bias model taken out --
    what ``new_user_embedding`` builds per query from ``BiasModel.compute_for_items``, bit for
    bit.  Returns (the residual CSR [B x items], int64 offsets from the host prefix sums as
    :func:`gather_rows` makes them, and the float64 user biases, device [B], 0 without a row).
    """
    lib = _native.require_gpu()
    hp = mat.h_indptr
    assert hp is not None and mat.values is not None and item_biases is not None
    assert item_biases.dtype == torch.float32 and int(item_biases.shape[0]) == mat.shape[1]
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    B = int(rows.shape[0])
    ok = (rows >= 0) & (rows < mat.shape[0])
    safe = np.where(ok, rows, 0)
    lens = np.where(ok, hp[safe + 1] - hp[safe], 0).astype(np.int64)
    ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    dev = mat.indices.device
    nnz = int(ptr[-1])
    packed = np.empty(2 * (B + 1) + B + (B & 1), dtype=np.int32)  # (one upload, as gather_rows)
    packed[:2 * (B + 1)] = ptr.view(np.int32)
    packed[2 * (B + 1):2 * (B + 1) + B] = rows
    d_packed = torch.from_numpy(packed).to(dev)
    d_ptr = d_packed[:2 * (B + 1)].view(torch.int64)
    d_rows = d_packed[2 * (B + 1):2 * (B + 1) + B]
    out_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(nnz, dtype=torch.float32, device=dev)
    ub = torch.zeros(B, dtype=torch.float64, device=dev)
    if B and nnz:  # (rows without an entry: nothing to write, and their bias is 0)
        check(
            lib.lk_bmf_residual_rows(
                _ptr(mat.indptr), 1 if mat.is64 else 0, _ptr(mat.indices), _ptr(mat.values),
                mat.shape[0], mat.shape[1], B, _ptr(d_rows), _ptr(d_ptr), float(global_bias),
                _ptr(item_biases), float(damping_user), _ptr(ub), _ptr(out_idx), _ptr(out_val),
                _stream()
            ),
            "lk_bmf_residual_rows",
        )  # fmt: skip
    return DeviceCSR(d_ptr, out_idx, out_val, (B, mat.shape[1]), ptr), ub


def _bmf_rows(panel: torch.Tensor, mode: torch.Tensor, ub: torch.Tensor, item_biases):
    rows, n_items = panel.shape
    assert panel.dtype == torch.float32 and panel.dim() == 2 and panel.is_contiguous()
    assert mode.dtype == torch.uint8 and mode.shape == (rows,) and mode.is_contiguous()
    assert ub.dtype == torch.float64 and ub.shape == (rows,) and ub.is_contiguous()
    assert item_biases.dtype == torch.float32 and item_biases.shape == (n_items,)
    return rows, n_items


def bmf_finish_panel(panel: torch.Tensor, mode: torch.Tensor, ub: torch.Tensor,
                     global_bias: float, item_biases: torch.Tensor,
                     strike_ptr: torch.Tensor | None = None,
                     strike_items: torch.Tensor | None = None) -> torch.Tensor:
    """
    ``BiasedMFScorer.finalize_scores`` in place on a [rows x items] f32 panel of
    :func:`score_dense` (lk_bmf_finish_panel): per row a mode (uint8, ``_native.BMF_*``) and a
    float64 user bias, the item biases f32 [items].  ``strike_ptr`` (int64 [rows + 1], offsets
    into ``strike_items``, int32): the row's listed items become NaN.  Returns ``panel``.
    """
    lib = _native.require_gpu()
    rows, n_items = _bmf_rows(panel, mode, ub, item_biases)
    if strike_ptr is not None:
        assert strike_ptr.dtype == torch.int64 and strike_ptr.shape == (rows + 1,)
        assert strike_items.dtype == torch.int32
    check(lib.lk_bmf_finish_panel(_ptr(panel), rows, n_items, n_items, _ptr(mode), _ptr(ub),
                                  float(global_bias), _ptr(item_biases), _ptr(strike_ptr),
                                  _ptr(strike_items), _stream()), "lk_bmf_finish_panel")
    return panel


def bmf_finish_pairs(panel: torch.Tensor, mode: torch.Tensor, ub: torch.Tensor,
                     global_bias: float, item_biases: torch.Tensor, tgt_ptr: torch.Tensor,
                     tgt_items: torch.Tensor, first: int, count: int,
                     out: torch.Tensor) -> torch.Tensor:
    """
    The same finish for ragged target lists (lk_bmf_finish_pairs): ``panel`` is the UNFINISHED
    :func:`score_dense` panel of the rows whose lists are ``tgt_ptr`` (int64 [rows + 1], absolute
    offsets into ``tgt_items`` int32 and ``out`` f32, ``tgt_ptr[0] == first``); the ``count``
    entries from ``first`` on are written to ``out`` (an unknown item, -1: NaN).
    """
    lib = _native.require_gpu()
    rows, n_items = _bmf_rows(panel, mode, ub, item_biases)
    assert tgt_ptr.dtype == torch.int64 and tgt_ptr.shape == (rows + 1,)
    assert tgt_items.dtype == torch.int32 and out.dtype == torch.float32
    assert 0 <= first and first + count <= min(int(tgt_items.shape[0]), int(out.shape[0]))
    check(lib.lk_bmf_finish_pairs(_ptr(panel), rows, n_items, n_items, _ptr(mode), _ptr(ub),
                                  float(global_bias), _ptr(item_biases), _ptr(tgt_ptr),
                                  _ptr(tgt_items), int(first), int(count), _ptr(out), _stream()),
          "lk_bmf_finish_pairs")
    return out


def iknn_recommend(sims: DeviceCSR, ref_ptr, ref_items, ref_rates, item_bias, max_nbrs: int,
                   min_nbrs: int, n: int, query_hits: np.ndarray, exclude_refs: bool = True):
    """
    Item-kNN top-``n`` recommendations for a batch of queries (lk_iknn_recommend): every item is
    scored with the reference accumulator's arithmetic (bit for bit), ``item_bias`` (the item
    means of the explicit model, device f32 [n_items], or None) is added, the query's own items
    are struck out (``exclude_refs``), and the ``n`` best scored items are returned.
    ``ref_ptr`` / ``ref_items`` / ``ref_rates``: device CSR-style history lists as for
    :func:`iknn_score_batch`; ``query_hits``: HOST int64 [queries], per query the summed
    similarity-row lengths of its history items (``item_counts[ref_items]`` summed per query).
    Returns device (item numbers int32 [B x n], -1 padded; scores f32 [B x n], NaN padded).
    """
    lib = _native.require_gpu()
    n_items = sims.shape[0]
    nq = int(ref_ptr.shape[0]) - 1
    dev = sims.indices.device
    assert sims.indptr.dtype == torch.int64
    query_hits = np.ascontiguousarray(query_hits, dtype=np.int64)
    assert query_hits.shape == (nq,)
    max_hits = int(query_hits.max()) if nq else 0
    cols = n_items if n < 0 else int(n)
    out_i = torch.empty((nq, cols), dtype=torch.int32, device=dev)
    out_s = torch.empty((nq, cols), dtype=torch.float32, device=dev)
    if nq == 0 or cols == 0:
        return out_i, out_s
    ws = torch.empty(lib.lk_iknn_recommend_workspace_bytes(n_items, nq, max_hits, int(max_nbrs),
                                                           int(n)),
                     dtype=torch.uint8, device=dev)
    check(
        lib.lk_iknn_recommend(
            _ptr(sims.indptr), _ptr(sims.indices), _ptr(sims.values), n_items, nq, _ptr(ref_ptr),
            _ptr(ref_items), _ptr(ref_rates), _ptr(item_bias), int(max_nbrs), int(min_nbrs),
            int(n), 1 if exclude_refs else 0, query_hits.ctypes.data_as(ctypes.c_void_p),
            max_hits, _ptr(ws), _ptr(out_i), _ptr(out_s), _stream()
        ),
        "lk_iknn_recommend",
    )  # fmt: skip
    return out_i, out_s


def knn_score_last_stats():
    "(queries on the candidate-list kernel, queries on the slot kernel, longest target list) of the last call"
    import ctypes

    out = (ctypes.c_int64 * 3)()
    _native.load().lk_knn_score_last_stats(out)
    return tuple(int(x) for x in out)


def uknn_score_batch(ratings: DeviceCSR, nbr_ptr, nbr_rows, nbr_sims, tgt_ptr, tgt_items,
                     max_nbrs: int, min_nbrs: int):
    """
    User-kNN scoring of a batch of queries (lk_uknn_score_batch; src/accel/knn/user_score.rs):
    ``ratings`` users x items CSR (int64 offsets; ``values`` None = implicit feedback),
    neighbours / targets as CSR-style (int64 offsets) lists.  Returns (scores, counts).
    """
    lib = _native.require_gpu()
    n_users, n_items = ratings.shape
    nq = int(nbr_ptr.shape[0]) - 1
    dev = ratings.indices.device
    assert ratings.indptr.dtype == torch.int64
    ws = torch.empty(lib.lk_iknn_score_workspace_bytes(n_items, nq, int(max_nbrs)),
                     dtype=torch.uint8, device=dev)
    out_s = torch.empty(int(tgt_items.shape[0]), dtype=torch.float32, device=dev)
    out_c = torch.empty(int(tgt_items.shape[0]), dtype=torch.int32, device=dev)
    check(
        lib.lk_uknn_score_batch(
            _ptr(ratings.indptr), _ptr(ratings.indices), _ptr(ratings.values), n_users, n_items,
            nq, _ptr(nbr_ptr), _ptr(nbr_rows), _ptr(nbr_sims), _ptr(tgt_ptr), _ptr(tgt_items),
            int(max_nbrs), int(min_nbrs), _ptr(ws), _ptr(out_s), _ptr(out_c), _stream()
        ),
        "lk_uknn_score_batch",
    )  # fmt: skip
    return out_s, out_c


def csr_rows_dot(csr: DeviceCSR, x: torch.Tensor) -> torch.Tensor:
    """
    ``out[q][r] = <row r of csr, x[:, q]>`` for the dense columns of ``x`` ([n_cols x B],
    row-major) -- the neighbour similarities of user-kNN (lk_csr_rows_dot).  Returns [B x rows].
    """
    lib = _native.require_gpu()
    n_rows, n_cols = csr.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == n_cols
    B = int(x.shape[1])
    out = torch.empty((B, n_rows), dtype=torch.float32, device=x.device)
    check(
        lib.lk_csr_rows_dot(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                            _ptr(csr.values), n_rows, _ptr(x), B, B, _ptr(out), n_rows,
                            _stream()),
        "lk_csr_rows_dot",
    )
    return out


def uknn_query_panel(hist: DeviceCSR, centre: torch.Tensor | None, *, ld: int | None = None,
                     rows: tuple[int, int] | None = None) -> torch.Tensor:
    """
    The dense query vectors of the histories ``hist`` (queries x items, int64 offsets, -1 =
    unknown item) built on the device (lk_uknn_query_panel): X [items x ld] f32, item-major as
    ``csr_rows_dot`` reads it.  With values: ``rating - centre[q]`` (``centre`` device f32 per
    query of ``hist``); without: 1.0.  A repeated item keeps its last occurrence.
    ``rows = (lo, hi)``: those queries only (column 0 is query ``lo``).
    """
    lib = _native.require_gpu()
    n_items = int(hist.shape[1])
    lo, hi = (0, int(hist.indptr.shape[0]) - 1) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= lo <= hi < int(hist.indptr.shape[0])
    P = hi - lo
    ld = P if ld is None else int(ld)
    assert ld >= P
    assert hist.indptr.dtype == torch.int64 and hist.indptr.is_contiguous()
    assert hist.indices.dtype == torch.int32 and hist.indices.is_contiguous()
    if hist.values is not None:
        assert hist.values.dtype == torch.float32 and hist.values.is_contiguous()
        assert centre is not None and centre.dtype == torch.float32 and centre.is_contiguous()
        assert centre.numel() == int(hist.indptr.shape[0]) - 1
        assert centre.device == hist.indices.device
    x = torch.empty((n_items, ld), dtype=torch.float32, device=hist.indices.device)
    if ld > P:
        x[:, P:] = 0.0
    check(
        lib.lk_uknn_query_panel(_ptr(hist.indptr[lo:]), _ptr(hist.indices), _ptr(hist.values),
                                _ptr(centre[lo:]) if hist.values is not None else None, P,
                                n_items, _ptr(x), ld, _stream()),
        "lk_uknn_query_panel",
    )
    return x


def uknn_sims_panel(vectors: DeviceCSR, x: torch.Tensor, self_user: torch.Tensor | None = None,
                    *, queries: int | None = None, ld: int | None = None) -> torch.Tensor:
    """
    ``sims[u][q] = <row u of vectors, x[:, q]>`` for the first ``queries`` columns of ``x``
    ([items x ld_x] f32), USER-major [users x ld] (lk_uknn_sims_panel): ``csr_rows_dot``'s bits,
    transposed.  ``self_user`` (device int32 per query, -1 = none): that entry is +0.0.
    """
    lib = _native.require_gpu()
    n_users, n_items = vectors.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    assert x.shape[0] == n_items and x.device == vectors.indices.device
    P = int(x.shape[1]) if queries is None else int(queries)
    assert 0 <= P <= int(x.shape[1])
    ld = P if ld is None else int(ld)
    assert ld >= P
    assert vectors.values is not None and vectors.values.dtype == torch.float32
    assert vectors.indices.dtype == torch.int32
    if self_user is not None:
        assert self_user.dtype == torch.int32 and self_user.is_contiguous()
        assert self_user.numel() == P and self_user.device == x.device
    out = torch.empty((n_users, ld), dtype=torch.float32, device=x.device)
    check(
        lib.lk_uknn_sims_panel(_ptr(vectors.indptr), 1 if vectors.is64 else 0,
                               _ptr(vectors.indices), _ptr(vectors.values), n_users, _ptr(x),
                               int(x.shape[1]), P, _ptr(self_user), _ptr(out), ld, _stream()),
        "lk_uknn_sims_panel",
    )
    return out


def uknn_lds_max_nbrs() -> int:
    "The largest ``max_nbrs`` whose accumulators ``lk_uknn_score_panel`` keeps in LDS."
    return int(_native.load().lk_uknn_score_panel_lds_max_nbrs())


def uknn_score_panel(ratings_t: DeviceCSR, sims: torch.Tensor, queries: int, thr: float,
                     max_nbrs: int, min_nbrs: int, offset: torch.Tensor | None = None, *,
                     hist: DeviceCSR | None = None, rows: tuple[int, int] | None = None,
                     strike_history: bool = False, nan_empty: bool = False,
                     item_order: torch.Tensor | None = None, max_col: int | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """
    The user-kNN score panel [queries x n_items] of ``lk_uknn_score_panel``, as ``argtopn`` wants
    it.  ``ratings_t``: the transposed centred ratings (items x users, int64 offsets, users
    ascending; ``values`` None = implicit feedback); ``sims``: the user-major panel of
    :func:`uknn_sims_panel` (its first ``queries`` columns); ``thr``: the float32 ``min_sim``;
    ``offset``: device f32 per query, added to explicit scores.  ``hist`` / ``rows = (lo, hi)``:
    the histories of the panel's queries are rows ``lo .. hi`` of ``hist``; ``strike_history``
    makes their items NaN, ``nan_empty`` the row of a query without a known item.
    ``item_order``: device int32 permutation of the items (heaviest column first);
    ``max_col``: the longest column (read from the device when not given).  ``out``: write into
    the first ``n_items`` columns of this [queries x ld] f32 device matrix (ld >= n_items) instead
    of a fresh panel; the other columns are left alone.
    """
    lib = _native.require_gpu()
    n_items, n_users = ratings_t.shape
    dev = sims.device
    P = int(queries)
    assert ratings_t.indptr.dtype == torch.int64 and ratings_t.indptr.is_contiguous()
    assert ratings_t.indices.dtype == torch.int32 and ratings_t.indices.device == dev
    assert ratings_t.values is None or (ratings_t.values.dtype == torch.float32 and
                                        ratings_t.values.is_contiguous())
    assert sims.dtype == torch.float32 and sims.is_contiguous() and sims.dim() == 2
    assert sims.shape[0] == n_users and 0 <= P <= int(sims.shape[1])
    if offset is not None:
        assert offset.dtype == torch.float32 and offset.is_contiguous() and offset.numel() == P
        assert offset.device == dev
    if item_order is not None:
        assert item_order.dtype == torch.int32 and item_order.is_contiguous()
        assert item_order.numel() == n_items and item_order.device == dev
    mark = (1 if strike_history else 0) | (2 if nan_empty else 0)
    h_ptr = h_idx = None
    if mark:
        assert hist is not None and hist.indptr.dtype == torch.int64
        assert hist.indices.dtype == torch.int32 and hist.indices.device == dev
        lo, hi = (0, int(hist.indptr.shape[0]) - 1) if rows is None else \
            (int(rows[0]), int(rows[1]))
        assert 0 <= lo <= hi < int(hist.indptr.shape[0]) and hi - lo == P
        h_ptr, h_idx = hist.indptr[lo:], hist.indices
    if max_col is None:
        max_col = int(torch.diff(ratings_t.indptr).max()) if n_items else 0
    if out is None:
        out = torch.empty((P, n_items), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.is_contiguous()
    assert out.shape[0] == P and out.shape[1] >= n_items and out.device == dev
    wb = lib.lk_uknn_score_panel_workspace_bytes(int(max_nbrs), int(max_col))
    ws = torch.empty(wb, dtype=torch.uint8, device=dev) if wb else None
    check(
        lib.lk_uknn_score_panel(_ptr(ratings_t.indptr), _ptr(ratings_t.indices),
                                _ptr(ratings_t.values), n_items, n_users, int(max_col),
                                _ptr(item_order), _ptr(sims), int(sims.shape[1]), P, float(thr),
                                int(max_nbrs), int(min_nbrs), _ptr(offset), _ptr(h_ptr),
                                _ptr(h_idx), mark, _ptr(ws), _ptr(out), int(out.shape[1]),
                                _stream()),
        "lk_uknn_score_panel",
    )
    return out


def uknn_pairs_lds_max_nbrs() -> int:
    "The largest ``max_nbrs`` whose accumulators ``lk_uknn_score_pairs`` keeps in LDS."
    return int(_native.load().lk_uknn_score_pairs_lds_max_nbrs())


def uknn_score_pairs(ratings_t: DeviceCSR, sims: torch.Tensor, tgt_ptr: torch.Tensor,
                     tgt_items: torch.Tensor, thr: float, max_nbrs: int, min_nbrs: int,
                     offset: torch.Tensor | None = None, *,
                     self_user: torch.Tensor | None = None, user_major: bool = False,
                     entries: tuple[int, int] | None = None, max_col: int | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """
    User-kNN scores of ragged (query, target) pairs (lk_uknn_score_pairs): what
    :func:`uknn_score_panel` writes into those cells, bit for bit.  ``ratings_t``: the transposed
    centred ratings (items x users, int64 offsets, users ascending; ``values`` None = implicit
    feedback); ``sims``: the query-major similarities [P x users] of :func:`csr_rows_dot`, or
    with ``user_major`` the panel [users x ld] of :func:`uknn_sims_panel` (its first P columns);
    ``tgt_ptr``: device int64 [P + 1], ABSOLUTE offsets into ``tgt_items`` (device int32, -1 =
    unknown item) -- a slice of a longer offset array is fine; ``thr``: the float32 ``min_sim``;
    ``offset``: device f32 per query, added to explicit scores; ``self_user``: device int32 per
    query (-1 = none), the rater that never passes.  ``entries = (lo, hi)``: the entries the
    ``P`` queries cover, when the caller knows them (else all of ``tgt_items``: only the launch
    is sized by it).  ``max_col``: the longest column (read from the device when not given).
    Returns ``out`` (f32, one score per entry of ``tgt_items``; NaN = cannot be scored); only
    the entries of the ``P`` queries are written.
    """
    lib = _native.require_gpu()
    n_items, n_users = ratings_t.shape
    dev = sims.device
    P = int(tgt_ptr.shape[0]) - 1
    total = int(tgt_items.shape[0])
    assert ratings_t.indptr.dtype == torch.int64 and ratings_t.indptr.is_contiguous()
    assert ratings_t.indices.dtype == torch.int32 and ratings_t.indices.device == dev
    assert ratings_t.values is None or (ratings_t.values.dtype == torch.float32 and
                                        ratings_t.values.is_contiguous())
    assert sims.dtype == torch.float32 and sims.is_contiguous() and sims.dim() == 2
    if user_major:
        assert P >= 0 and sims.shape[0] == n_users and sims.shape[1] >= P
    else:
        assert P >= 0 and sims.shape[0] >= P and sims.shape[1] >= n_users
    assert tgt_ptr.dtype == torch.int64 and tgt_ptr.is_contiguous() and tgt_ptr.device == dev
    assert tgt_items.dtype == torch.int32 and tgt_items.is_contiguous()
    assert tgt_items.device == dev
    if offset is not None:
        assert offset.dtype == torch.float32 and offset.is_contiguous() and offset.numel() == P
        assert offset.device == dev
    if self_user is not None:
        assert self_user.dtype == torch.int32 and self_user.is_contiguous()
        assert self_user.numel() == P and self_user.device == dev
    lo, hi = (0, total) if entries is None else (int(entries[0]), int(entries[1]))
    assert 0 <= lo <= hi <= total
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == total
    assert out.device == dev
    if max_col is None:
        max_col = int(torch.diff(ratings_t.indptr).max()) if n_items else 0
    wb = lib.lk_uknn_score_pairs_workspace_bytes(int(max_nbrs), int(max_col))
    ws = torch.empty(wb, dtype=torch.uint8, device=dev) if wb else None
    check(
        lib.lk_uknn_score_pairs(_ptr(ratings_t.indptr), _ptr(ratings_t.indices),
                                _ptr(ratings_t.values), n_items, n_users, int(max_col),
                                _ptr(sims), int(sims.shape[1]), 1 if user_major else 0, P,
                                _ptr(self_user),
                                _ptr(tgt_ptr), _ptr(tgt_items), lo, hi - lo, float(thr),
                                int(max_nbrs), int(min_nbrs), _ptr(offset), _ptr(ws), _ptr(out),
                                _stream()),
        "lk_uknn_score_pairs",
    )
    return out


def ease_gram(cooc: DeviceCSR, item_counts: torch.Tensor, reg: float) -> torch.Tensor:
    """
    ``X^T X + reg I`` as a dense [n x n] f32 device matrix (lk_ease_gram) from the off-diagonal
    co-occurrence counts (``iknn_build`` of the binary matrix, threshold 0.5) and the item counts.
    """
    lib = _native.require_gpu()
    n = int(cooc.shape[0])
    out = torch.empty((n, n), dtype=torch.float32, device=cooc.indices.device)
    assert cooc.indptr.dtype == torch.int64 and item_counts.dtype == torch.int32
    check(
        lib.lk_ease_gram(_ptr(cooc.indptr), _ptr(cooc.indices), _ptr(cooc.values),
                         _ptr(item_counts), n, float(reg), _ptr(out), n, _stream()),
        "lk_ease_gram",
    )
    return out


def ease_score_batch(hist_ptr: torch.Tensor, hist_items: torch.Tensor,
                     weights: torch.Tensor) -> torch.Tensor:
    "Sum of the history items' weight rows per query, [B x n_items] f32 (lk_ease_score_batch)."
    lib = _native.require_gpu()
    n = int(weights.shape[0])
    B = int(hist_ptr.shape[0]) - 1
    assert hist_ptr.dtype == torch.int64 and hist_items.dtype == torch.int32
    assert weights.dtype == torch.float32 and weights.is_contiguous()
    out = torch.empty((B, n), dtype=torch.float32, device=weights.device)
    for lo in range(0, B, 65535):
        hi = min(B, lo + 65535)
        check(
            lib.lk_ease_score_batch(_ptr(hist_ptr[lo:]), _ptr(hist_items), hi - lo,
                                    _ptr(weights), n, n, _ptr(out[lo:]), n, _stream()),
            "lk_ease_score_batch",
        )
    return out


def ease_score_panel(hist_ptr: torch.Tensor, hist_items: torch.Tensor, weights: torch.Tensor,
                     rows: tuple[int, int] | None = None, strike_history: bool = False,
                     nan_empty: bool = False) -> torch.Tensor:
    """
    ``ease_score_batch`` as a panel for ``argtopn`` (lk_ease_score_panel): the sum of the history
    items' rows of the dense ``weights`` in history order, -1 (unknown) adding nothing, [B x
    n_items] f32 with the bits ``ease_score_batch`` gives; any number of queries.  ``rows = (lo,
    hi)``: those queries only.  ``strike_history`` makes the query's own items NaN, ``nan_empty``
    the whole row of a query without a known item.
    """
    lib = _native.require_gpu()
    n = int(weights.shape[0])
    lo, hi = (0, int(hist_ptr.shape[0]) - 1) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= lo <= hi < int(hist_ptr.shape[0])
    assert hist_ptr.dtype == torch.int64 and hist_items.dtype == torch.int32
    assert weights.dtype == torch.float32 and weights.is_contiguous()
    out = torch.empty((hi - lo, n), dtype=torch.float32, device=weights.device)
    check(
        lib.lk_ease_score_panel(_ptr(hist_ptr[lo:]), _ptr(hist_items), hi - lo, _ptr(weights), n,
                                n, _ptr(out), n, (1 if strike_history else 0) |
                                (2 if nan_empty else 0), _stream()),
        "lk_ease_score_panel",
    )
    return out


def gemm_tile() -> int:
    "The tile ``gemm_f32``'s masks count in (lk_gemm_tile)."
    return int(_native.load().lk_gemm_tile())


def gemm_f32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, *, trans_a: bool = False,
             trans_b: bool = False, alpha: float = 1.0, beta: float = 0.0,
             mask: int = 0) -> torch.Tensor:
    """
    ``c <- beta c + alpha op(a) op(b)`` in place (lk_gemm_f32): 2-D float32 device tensors whose
    rows are contiguous (any row stride: views of larger matrices are fine), ``op`` the transpose
    where ``trans_*``.  ``mask``: ``_native.GEMM_LOWER`` / ``GEMM_K_FROM_COL`` / ``GEMM_K_FROM_ROW``
    in tiles of :func:`gemm_tile`.  Returns ``c``.
    """
    lib = _native.require_gpu()
    for t in (a, b, c):
        assert t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)
    m, n = int(c.shape[0]), int(c.shape[1])
    k = int(a.shape[0] if trans_a else a.shape[1])
    assert tuple(a.shape) == ((k, m) if trans_a else (m, k))
    assert tuple(b.shape) == ((n, k) if trans_b else (k, n))

    def ld(t):  # (the stride of a one-row view is arbitrary: give the row length)
        return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])

    check(
        lib.lk_gemm_f32(int(trans_a), int(trans_b), m, n, k, float(alpha), _ptr(a), ld(a),
                        _ptr(b), ld(b), float(beta), _ptr(c), ld(c), int(mask), _stream()),
        "lk_gemm_f32",
    )
    return c


def spd_inverse_blocked_max_n() -> int:
    "The largest matrix ``spd_inverse_blocked`` accepts (lk_spd_inverse_blocked_max_n)."
    return int(_native.load().lk_spd_inverse_blocked_max_n())


def spd_inverse_blocked(a: torch.Tensor, flag: torch.Tensor | None = None):
    """
    The inverse of the SPD matrix ``a`` IN PLACE (lk_spd_inverse_blocked: blocked Cholesky, f32
    MFMA GEMMs, float64 diagonal blocks): a square float32 device matrix, or a square view with
    contiguous rows of a wider one.  Everything is queued on the current stream; the workspace
    (a second matrix and panels) is released on return, stream-ordered.  Returns (``a``, the int32
    device flag: 0, or 1 + the first block that is not positive definite -- ``a`` is then zeros).
    The caller reads the flag.
    """
    lib = _native.require_gpu()
    assert a.dtype == torch.float32 and a.dim() == 2 and a.shape[0] == a.shape[1]
    n = int(a.shape[0])
    assert n <= 1 or a.stride(1) == 1
    if n > spd_inverse_blocked_max_n():
        raise ValueError(f"spd_inverse_blocked: n = {n} above {spd_inverse_blocked_max_n()}")
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=a.device)
    nbytes = int(lib.lk_spd_inverse_blocked_workspace_bytes(n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=a.device)
    check(
        lib.lk_spd_inverse_blocked(_ptr(a), n, max(int(a.stride(0)), n) if n > 1 else n, _ptr(ws),
                                   nbytes, _ptr(flag), _stream()),
        "lk_spd_inverse_blocked",
    )
    return a, flag


SLIM_STAGE_BYTES = 2 << 30  # staging area of one lk_slim_train_count call (column batches)


def slim_train(ui: DeviceCSR, iu: DeviceCSR, l1: float, l2: float, max_iters: int,
               max_nbrs: int | None, columns=None, ctl: "TaskCtl | None" = None,
               stats: dict | None = None, on_batch=None) -> DeviceCSR:
    """
    SLIM / fsSLIM training (lk_slim_train_count / _fill; ``train_slim``,
    src/accel/slim/mod.rs:58-301): ``ui`` users x items and ``iu`` items x users, structure only
    (values are ignored).  Returns the rows of the TRANSPOSED weight matrix for the target items
    ``columns`` (host integers; None = every item) as a device CSR with int64 offsets, rows in
    the order of the list (item order for None), columns ascending -- the reference's rows bit
    for bit.  Long column
    lists go through in batches whose staging area stays under ``SLIM_STAGE_BYTES``;
    ``on_batch(columns done)`` is called after each.  ``stats``: receives the summed
    ``rounds``, ``coord_updates`` and ``resid_entries`` of the descent.
    """
    lib = _native.require_gpu()
    n_users, n_items = ui.shape
    assert iu.shape == (n_items, n_users)
    assert ui.h_indptr.dtype == iu.h_indptr.dtype
    if int(max_iters) < 1:
        raise ValueError("max_iters must be positive")
    dev = ui.indices.device
    is64 = 1 if ui.h_indptr.dtype == np.int64 else 0
    mn = 0 if max_nbrs is None else int(max_nbrs)
    if max_nbrs is not None and mn < 1:
        raise ValueError("max_nbrs must be positive")
    if columns is None:
        cols = None
        n_cols = n_items
    else:
        cols = np.ascontiguousarray(columns, dtype=np.int32)
        if cols.ndim != 1 or (len(cols) and (cols.min() < 0 or cols.max() >= n_items)):
            raise ValueError("slim_train: column out of range")
        n_cols = len(cols)
    if n_cols == 0:
        return DeviceCSR(torch.zeros(1, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev),
                         torch.empty(0, dtype=torch.float32, device=dev), (0, n_items), None)
    # sqrt(n_j) as the reference forms it, (n as f64).sqrt(): NumPy's sqrt is correctly rounded
    sq = torch.from_numpy(np.sqrt(np.diff(iu.h_indptr).astype(np.float64))).to(dev)
    cap = min(mn, n_items) if mn else n_items
    step = max(1, SLIM_STAGE_BYTES // (8 * max(cap, 1)))
    order = None
    if cols is None and n_items > 1:
        # every column: the most-rated targets first -- their columns are the long ones, and the
        # waves draw columns in list order -- and the rows put back in item order at the end
        order = np.argsort(-np.diff(iu.h_indptr), kind="stable").astype(np.int32)
        cols = order
    tot = {"rounds": 0, "coord_updates": 0, "resid_entries": 0}
    parts = []
    for lo in range(0, max(n_cols, 1), step):
        hi = min(n_cols, lo + step)
        nb = hi - lo
        d_cols = None if cols is None else torch.from_numpy(cols[lo:hi]).to(dev)
        ws = torch.empty(lib.lk_slim_train_workspace_bytes(n_users, n_items, nb, mn),
                         dtype=torch.uint8, device=dev)
        out_ptr = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        total = ctypes.c_int64(0)
        st = (ctypes.c_int64 * 3)()
        check(
            lib.lk_slim_train_count(
                _ptr(ui.indptr), _ptr(ui.indices), _ptr(iu.indptr), _ptr(iu.indices), is64,
                n_users, n_items, _ptr(sq), float(np.float32(l1)), float(np.float32(l2)),
                int(max_iters), mn, _ptr(d_cols), nb, None if ctl is None else ctl._h, _ptr(ws),
                _ptr(out_ptr), ctypes.byref(total), st, _stream()
            ),
            "lk_slim_train_count",
        )  # fmt: skip
        nnz = int(total.value)
        out_idx = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        out_val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)[:nnz]
        if nnz:
            check(
                lib.lk_slim_train_fill(n_users, n_items, nb, mn, _ptr(ws), _ptr(out_ptr),
                                       _ptr(out_idx), _ptr(out_val), _stream()),
                "lk_slim_train_fill",
            )
        torch.cuda.current_stream().synchronize()
        del ws
        for k, v in zip(tot, st):
            tot[k] += int(v)
        parts.append((out_ptr, out_idx, out_val))
        if on_batch is not None:
            on_batch(hi)
    if stats is not None:
        stats.update(tot)
    if len(parts) == 1:
        ptr, idx, val = parts[0]
    else:  # (plumbing: the batches' rows one after the other)
        base, ptrs = 0, [parts[0][0][:1]]
        for p, _i, _v in parts:
            ptrs.append(p[1:] + base)
            base += int(p[-1])
        ptr = torch.cat(ptrs)
        idx = torch.cat([p[1] for p in parts])
        val = torch.cat([p[2] for p in parts])
    out = DeviceCSR(ptr, idx, val, (n_cols, n_items), None)
    if order is not None:
        out.h_indptr = ptr.cpu().numpy()
        inv = np.empty_like(order)
        inv[order] = np.arange(n_items, dtype=np.int32)
        out = gather_rows(out, inv)
        out.h_indptr = None
    return out


def slim_score_batch(hist_ptr: torch.Tensor, hist_items: torch.Tensor, weights: DeviceCSR,
                     rows: tuple[int, int] | None = None, strike_history: bool = False,
                     nan_empty: bool = False) -> torch.Tensor:
    """
    ``x @ weights`` per query (lk_slim_score_batch; src/lenskit/knn/slim.py:139-144): the history
    items' rows of the stored ``weights`` CSR (int64 offsets) added in history order into a dense
    [B x n_items] f32 panel; unreached items are 0.  ``rows = (lo, hi)``: those queries only.
    The panel as ``argtopn`` wants it: ``strike_history`` makes the query's own items NaN,
    ``nan_empty`` the whole row of a query with an empty history.
    """
    lib = _native.require_gpu()
    n = int(weights.shape[1])
    lo, hi = (0, int(hist_ptr.shape[0]) - 1) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= lo <= hi < int(hist_ptr.shape[0])
    assert hist_ptr.dtype == torch.int64 and hist_items.dtype == torch.int32
    assert weights.indptr.dtype == torch.int64
    out = torch.empty((hi - lo, n), dtype=torch.float32, device=weights.indices.device)
    check(
        lib.lk_slim_score_batch(_ptr(hist_ptr[lo:]), _ptr(hist_items), hi - lo,
                                _ptr(weights.indptr), _ptr(weights.indices), _ptr(weights.values),
                                n, _ptr(out), n, (1 if strike_history else 0) |
                                (2 if nan_empty else 0), _stream()),
        "lk_slim_score_batch",
    )
    return out


def assoc_window() -> int:
    "The most item columns one workgroup of ``lk_assoc_score_batch`` accumulates (lk_assoc_window)."
    return int(_native.load().lk_assoc_window())


def assoc_scale(cooc: DeviceCSR, item_counts: torch.Tensor, n_groups: int, method: str,
                damping: float) -> DeviceCSR:
    """
    Co-occurrence counts -> association scores, IN PLACE (lk_assoc_scale;
    src/lenskit/knn/association.py:110-124): ``cooc`` is the square CSR ``iknn_build`` returns for
    the binary matrix (int64 offsets, threshold 0.5), ``item_counts`` the items' int32 interaction
    counts on the device, ``n_groups`` the interaction matrix's row count.  ``method``:
    ``"probability"`` or ``"lift"``.  Returns ``cooc``.
    """
    lib = _native.require_gpu()
    n = int(cooc.shape[0])
    if method not in _native.ASSOC_METHODS:
        raise ValueError(f"assoc_scale: unknown method {method!r}")
    assert cooc.shape[1] == n and cooc.indptr.dtype == torch.int64
    assert cooc.values is not None and cooc.values.dtype == torch.float32
    assert item_counts.dtype == torch.int32 and item_counts.numel() == n
    check(
        lib.lk_assoc_scale(_ptr(cooc.indptr), _ptr(cooc.indices), _ptr(cooc.values),
                           _ptr(item_counts), n, int(n_groups), _native.ASSOC_METHODS[method],
                           float(damping), _stream()),
        "lk_assoc_scale",
    )
    return cooc


def assoc_score_batch(ref_ptr: torch.Tensor, ref_items: torch.Tensor, s: DeviceCSR,
                      reduce: str, rows: tuple[int, int] | None = None,
                      strike_history: bool = False, nan_empty: bool = True,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """
    The mean or the maximum of the reference items' rows of the association matrix ``s`` per query
    (lk_assoc_score_batch; src/lenskit/knn/association.py:149-153), a dense [B x n_items] f32
    panel: reference items in the order given, repeats counted, -1 (unknown) skipped, absent cells
    0.  ``reduce``: ``"mean"`` or ``"max"``.  ``rows = (lo, hi)``: those queries only.  The panel
    as ``argtopn`` wants it: ``strike_history`` makes the query's own items NaN, ``nan_empty`` the
    whole row of a query without a known reference item (else it is 0).  ``out``: write into
    the first ``n_items`` columns of this [hi - lo x ld] f32 device matrix (ld >= n_items) instead
    of a fresh panel; the other columns are left alone.
    """
    lib = _native.require_gpu()
    n = int(s.shape[1])
    if reduce not in _native.ASSOC_REDUCTIONS:
        raise ValueError(f"assoc_score_batch: unknown reduction {reduce!r}")
    lo, hi = (0, int(ref_ptr.shape[0]) - 1) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= lo <= hi < int(ref_ptr.shape[0])
    assert ref_ptr.dtype == torch.int64 and ref_items.dtype == torch.int32
    assert s.indptr.dtype == torch.int64 and s.shape[0] == n
    if out is None:
        out = torch.empty((hi - lo, n), dtype=torch.float32, device=s.indices.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.is_contiguous()
    assert out.shape[0] == hi - lo and out.shape[1] >= n
    check(
        lib.lk_assoc_score_batch(_ptr(ref_ptr[lo:]), _ptr(ref_items), hi - lo, _ptr(s.indptr),
                                 _ptr(s.indices), _ptr(s.values), n,
                                 _native.ASSOC_REDUCTIONS[reduce], _ptr(out), int(out.shape[1]),
                                 (1 if strike_history else 0) | (2 if nan_empty else 0),
                                 _stream()),
        "lk_assoc_score_batch",
    )
    return out


def take_scores(scores: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    "The scores of the lists ``argtopn`` selected: [B x n] f32, NaN under -1 (lk_take_scores)."
    lib = _native.require_gpu()
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 2
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape[0] == scores.shape[0]
    out = torch.empty(tuple(idx.shape), dtype=torch.float32, device=scores.device)
    check(lib.lk_take_scores(_ptr(scores), scores.shape[0], scores.shape[1], _ptr(idx),
                             idx.shape[1], _ptr(out), _stream()), "lk_take_scores")
    return out


def shared_order_topn(order: torch.Tensor, order_scores: torch.Tensor, n: int, rows_out: int, *,
                      hist: DeviceCSR | None = None, rows: torch.Tensor | None = None):
    """
    ``rows_out`` top-N lists from one shared order (lk_shared_order_topn): list b is the first
    ``n`` entries of ``order`` (device int32 [L], with ``order_scores`` f32 [L]) that are not in
    row ``rows[b]`` of ``hist`` (device int32 [rows_out], -1 = no history; None: row b) -- a CSR
    of item-sorted rows, either offset width; ``hist=None``: nothing is skipped.  Returns device
    (item numbers int32 [rows_out x width], scores f32 [rows_out x width]) with -1 / NaN padding,
    width = ``n`` (``n < 0``: L).
    """
    lib = _native.require_gpu()
    assert order.dtype == torch.int32 and order.is_contiguous() and order.dim() == 1
    assert order_scores.dtype == torch.float32 and order_scores.is_contiguous()
    assert order_scores.shape == order.shape
    L, n, B = int(order.shape[0]), int(n), int(rows_out)
    width = L if n < 0 else n
    dev = order.device
    idx = torch.empty((B, width), dtype=torch.int32, device=dev)
    sc = torch.empty((B, width), dtype=torch.float32, device=dev)
    if B == 0 or width == 0:
        return idx, sc
    ptr = ind = None
    n_hist = 0
    if hist is not None and hist.indices.numel() == 0:
        hist = rows = None  # (a CSR without entries: nothing to skip, and no address to pass)
    if hist is not None:
        ptr, ind, n_hist = hist.indptr, hist.indices, int(hist.shape[0])
        assert ptr.dtype in (torch.int32, torch.int64) and ptr.is_contiguous()
        assert ptr.shape == (n_hist + 1,) and ind.dtype == torch.int32 and ind.is_contiguous()
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.shape == (B,)
    else:
        assert hist is None or n_hist >= B
    check(lib.lk_shared_order_topn(_ptr(order), _ptr(order_scores), L, _ptr(ptr),
                                   1 if (ptr is not None and ptr.dtype == torch.int64) else 0,
                                   _ptr(ind), n_hist, _ptr(rows), B, n, _ptr(idx), _ptr(sc),
                                   _stream()), "lk_shared_order_topn")
    return idx, sc


def score_dense(users: torch.Tensor, items: torch.Tensor, k: int) -> torch.Tensor:
    "All (user, item) scores, [B x I] f32 (lk_score_dense)."
    lib = _native.require_gpu()
    B, kp = users.shape
    I = items.shape[0]
    assert kp == padded_dim(k) and items.shape[1] == kp
    out = torch.empty((B, I), dtype=torch.float32, device=users.device)
    check(
        lib.lk_score_dense(_ptr(users), kp, B, _ptr(items), kp, I, int(k), _ptr(out), I, _stream()),
        "lk_score_dense",
    )
    return out


def _row_streams(streams, rows: int, dev) -> torch.Tensor:
    "uint64 [rows] stream numbers (NumPy, or a device int64 tensor holding the bits) in HBM"
    if isinstance(streams, torch.Tensor):
        assert streams.dtype == torch.int64 and streams.is_contiguous()
        streams = streams.to(dev)
    else:
        host = np.ascontiguousarray(streams, dtype=np.uint64).reshape(-1)
        streams = torch.from_numpy(host.view(np.int64)).to(dev)
    assert streams.shape == (rows,)
    return streams


def stochastic_keys(panel: torch.Tensor, streams, *, transform, scale: float, seed: int,
                    sample: int = 0, excl=None, stats: torch.Tensor | None = None,
                    out: torch.Tensor | None = None):
    """
    The sort keys of the stochastic ranker (lk_stochastic_row_stats, lk_stochastic_keys) for a
    [rows x len] f32 device panel of scores (rows ``stride(0)`` apart): ``argtopn`` of a key row is
    one sampled ranking.  ``streams``: uint64 [rows]; ``seed``: 64 bits; ``excl``: a ``DeviceCSR``
    or (int64 offsets, int32 sorted items) whose entries take no part.  ``stats`` from an earlier
    call on the same panel skips the statistics pass (the samples of one call share it); ``out``:
    a contiguous [rows x len] f32 buffer to write the keys into.  Returns (keys, stats): stats is
    [rows x 4] f32 -- max, min, sum, and the count's int32 bits.
    """
    lib = _native.require_gpu()
    assert panel.dtype == torch.float32 and panel.dim() == 2
    rows, ln = panel.shape
    assert ln <= 1 or panel.stride(1) == 1
    ld = panel.stride(0) if rows > 1 and ln > 0 else max(ln, 1)
    assert ld >= ln
    dev = panel.device
    code = _native.STOCHASTIC_TRANSFORMS[transform]
    ptr = items = None
    if excl is not None:
        ptr, items = (excl.indptr, excl.indices) if isinstance(excl, DeviceCSR) else excl
        assert ptr.dtype == torch.int64 and items.dtype == torch.int32 and ptr.shape == (rows + 1,)
    if stats is None:
        stats = torch.empty((rows, 4), dtype=torch.float32, device=dev)
        check(lib.lk_stochastic_row_stats(_ptr(panel), rows, ln, ld, _ptr(ptr), _ptr(items), code,
                                          float(scale), _ptr(stats), _stream()),
              "lk_stochastic_row_stats")
    assert stats.shape == (rows, 4) and stats.is_contiguous()
    if out is None:
        out = torch.empty((rows, ln), dtype=torch.float32, device=dev)
    assert out.shape == (rows, ln) and out.is_contiguous() and out.dtype == torch.float32
    check(lib.lk_stochastic_keys(_ptr(panel), rows, ln, ld, _ptr(ptr), _ptr(items), code,
                                 float(scale), _ptr(stats), int(seed) & (2**64 - 1),
                                 _ptr(_row_streams(streams, rows, dev)), int(sample), _ptr(out), ln,
                                 _stream()), "lk_stochastic_keys")
    return out, stats


def stochastic_key_of_bits(log_weight: torch.Tensor, bits: torch.Tensor) -> torch.Tensor:
    "The key function on given random words (lk_stochastic_key_of_bits); ``bits``: int32 bits."
    lib = _native.require_gpu()
    assert log_weight.dtype == torch.float32 and bits.dtype == torch.int32
    assert log_weight.is_contiguous() and bits.is_contiguous() and log_weight.shape == bits.shape
    out = torch.empty_like(log_weight)
    check(lib.lk_stochastic_key_of_bits(_ptr(log_weight), _ptr(bits), log_weight.numel(),
                                        _ptr(out), _stream()), "lk_stochastic_key_of_bits")
    return out


def fold_in(hist: DeviceCSR, items: torch.Tensor, otor: torch.Tensor, k: int,
            solver: int = _native.SOLVER_AUTO, pending: list | None = None) -> torch.Tensor:
    """
    Batched new-user embeddings (``ImplicitMFScorer._train_new_row``,
    src/lenskit/als/_implicit.py:101-130): one ALS row solve per history row of ``hist``
    (queries x items CSR, values = weight or weight*rating) against ``items`` and
    ``otor`` = Q^T Q + user_reg I.  Returns [n_queries x KP]; empty histories give zeros.
    ``pending``: the launch is left unchecked and its plan appended there -- the caller runs
    ``check_status`` once its own launches are queued behind this one (no host wait in between).

    The plan sums in the kernels' own (``accurate``) order whatever ``LK_ALS_RHS_ORDER`` says for
    training: the hybrid order reproduces the RUST half-epoch's sequential float32 sums
    (src/accel/als/implicit.rs:110-117), but a fold-in is the reference's PYTHON path --
    ``(M.T * ratings) @ M`` and ``M.T @ (ratings + 1)`` through NumPy's BLAS, ``cho_factor`` -- which
    has no such chain.  Measured on 10 000 ML-25M-shaped histories against that restatement
    (``oracle.als_fold_in``): worst row 3.0e-5 / median 2.2e-6 in this order, 4.0e-5 / 2.7e-6 in the
    hybrid one; and the launch is 0.24 instead of 0.29 ms (no chain kernel, no slab sums).
    """
    plan = ALSPlan(hist, k, solver, reference_order="accurate")
    out = torch.zeros((hist.shape[0], plan.kp), dtype=torch.float32, device=items.device)
    plan.half_epoch(out, items, otor)
    if pending is None:
        plan.check_status()
    else:
        pending.append(plan)
    return out


def fold_in_explicit(hist: DeviceCSR, items: torch.Tensor, reg: float, k: int,
                     pending: list | None = None) -> torch.Tensor:
    """
    Batched new-user embeddings of the biased-MF model (``_train_bias_row_cholesky``,
    src/lenskit/als/_explicit.py:121-149): one explicit row solve per history row of ``hist``
    (queries x items CSR, values = bias-normalised ratings).  Returns [n_queries x KP]; empty
    histories give zeros.  ``pending``: as :func:`fold_in` -- the launch is left unchecked and its
    plan appended there, for the caller to check once its own launches are queued behind it.
    """
    plan = ALSPlan(hist, k, _native.SOLVER_CHOLESKY, reference_order="accurate")  # (as fold_in)
    out = torch.zeros((hist.shape[0], plan.kp), dtype=torch.float32, device=items.device)
    plan.half_epoch_explicit(out, items, reg)
    if pending is None:
        plan.check_status()
    else:
        pending.append(plan)
    return out


def gather_rows(csr: DeviceCSR, rows: np.ndarray, *, scale: float = 1.0,
                with_values: bool = True, col_bias: torch.Tensor | None = None) -> DeviceCSR:
    """
    The rows ``rows`` (HOST int32, -1 = an empty row) of a device CSR as a new device CSR with
    int64 offsets (lk_csr_gather_rows): the histories of a batch of queries cut out of the
    training matrix in one launch (src/lenskit/basic/history.py:37-95 per query in the
    reference).  Values are ``csr.values * scale`` in float32, or the constant ``scale`` when the
    matrix holds none (src/lenskit/als/_implicit.py:83-92); ``col_bias`` (device f32 per column)
    is subtracted before the scaling (item.py:268-271); ``with_values=False``: structure only.  The offsets are prefix sums of the host copy of ``csr``'s offsets: a few thousand
    integers on the host, nothing of the size of the matrix.
    """
    lib = _native.require_gpu()
    hp = csr.h_indptr
    assert hp is not None, "gather_rows needs the host copy of the offsets"
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    B = int(rows.shape[0])
    safe = np.where(rows >= 0, rows, 0)
    lens = np.where(rows >= 0, hp[safe + 1] - hp[safe], 0).astype(np.int64)
    ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    dev = csr.indices.device
    nnz = int(ptr[-1])
    # one upload for the two small host arrays (offsets, row numbers)
    packed = np.empty(2 * (B + 1) + B + (B & 1), dtype=np.int32)
    packed[:2 * (B + 1)] = ptr.view(np.int32)
    packed[2 * (B + 1):2 * (B + 1) + B] = rows
    d_packed = torch.from_numpy(packed).to(dev)
    d_ptr = d_packed[:2 * (B + 1)].view(torch.int64)
    d_rows = d_packed[2 * (B + 1):2 * (B + 1) + B]
    out_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(nnz, dtype=torch.float32, device=dev) if with_values else None
    if B and nnz:
        check(
            lib.lk_csr_gather_rows(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                                   _ptr(csr.values), B, _ptr(d_rows), _ptr(d_ptr), _ptr(col_bias),
                                   float(np.float32(scale)), _ptr(out_idx), _ptr(out_val),
                                   _stream()),
            "lk_csr_gather_rows",
        )
    return DeviceCSR(d_ptr, out_idx, out_val, (B, csr.shape[1]), ptr)


def csr_transpose(csr: DeviceCSR, with_values: bool = True) -> DeviceCSR:
    """
    Stable transpose on the device (lk_csr_transpose; ``SparseRowArray.transpose`` /
    ``_accel.data.transpose_csr``, src/lenskit/data/matrix.py:512-530,
    src/accel/data/transpose.rs:19-108): entries of an output row keep the input's entry
    order, i.e. ascending source row.  Offsets keep the input's width.
    """
    lib = _native.require_gpu()
    n_rows, n_cols = csr.shape
    nnz = int(csr.indices.shape[0])
    dev = csr.indices.device
    is64 = 1 if csr.indptr.dtype == torch.int64 else 0
    wb = lib.lk_csr_transpose_workspace_bytes(nnz, n_cols, is64)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    t_ptr = torch.empty(n_cols + 1, dtype=csr.indptr.dtype, device=dev)
    t_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    perm = torch.empty(nnz, dtype=csr.indptr.dtype, device=dev) if with_values else None
    check(
        lib.lk_csr_transpose(_ptr(csr.indptr), is64, _ptr(csr.indices), n_rows, n_cols, nnz,
                             _ptr(t_ptr), _ptr(t_idx), _ptr(perm), _ptr(ws), wb, _stream()),
        "lk_csr_transpose",
    )
    vals = csr.values[perm.long()] if with_values and csr.values is not None else None
    out = DeviceCSR(t_ptr, t_idx, vals, (n_cols, n_rows), None)
    out.perm = perm
    return out


def iknn_prepare(ratings, explicit: bool = True, dev=None):
    """
    Item-kNN rating normalisation (``ItemKNNScorer._center_ratings`` / ``_normalize_rows``,
    src/lenskit/knn/item.py:202-228) with the data on the device: ``ratings`` is the
    users x items matrix (SciPy; for implicit feedback the caller passes the interaction
    matrix of ones, like the reference) and ``explicit`` selects the item-mean centring.
    Returns (ui DeviceCSR, iu DeviceCSR, item means | None, all_zero flag) -- the two
    orientations the similarity build consumes -- bit-identical to the reference's SciPy
    preparation: the structure comes from the stable device transpose, every elementwise
    step and the sequential sum of squares from csrc/iknn_prepare.hip, and the two per-item
    vectors whose rounding depends on the host's NumPy (``np.add.reduceat`` sums, sqrt /
    reciprocal of the norms) from the very calls the reference makes, on [n_items] arrays.
    """
    import scipy.sparse as sps

    lib = _native.require_gpu()
    dev = device(dev)
    csr = sps.csr_array(ratings).astype(np.float32)
    csr.sort_indices()
    n_users, n_items = csr.shape
    dcsr = DeviceCSR.from_arrays(csr.indptr, csr.indices, csr.data, csr.shape, dev)
    t = csr_transpose(dcsr)  # item-major values, offsets, users, permutation
    is64 = 1 if t.indptr.dtype == torch.int64 else 0
    t_ptr = t.indptr.cpu().numpy()
    counts = np.diff(t_ptr)
    means = d_means = None
    if explicit:
        # rmat.sum(axis=0) on the CSC matrix == np.add.reduceat over the non-empty items
        # (scipy.sparse._compressed._cs_matrix.sum -> _minor_reduce), in the host's NumPy
        vals_items = t.values.cpu().numpy()
        nonempty = np.flatnonzero(counts)
        sums = np.zeros(n_items, dtype=np.float32)
        if len(nonempty):
            sums[nonempty] = np.add.reduceat(vals_items, t_ptr[nonempty])
        means = np.zeros(n_items, dtype=np.float32)
        np.divide(sums, counts, out=means, where=counts > 0)
        d_means = torch.from_numpy(means).to(dev)
    nnz = t.nnz
    cent = torch.empty(nnz, dtype=torch.float32, device=dev)
    sumsq = torch.empty(n_items, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    check(
        lib.lk_iknn_prep_center(_ptr(t.indptr), is64, _ptr(t.values), _ptr(d_means), n_items,
                                _ptr(cent), _ptr(sumsq), _ptr(flag), _stream()),
        "lk_iknn_prep_center",
    )
    norms = np.sqrt(sumsq.cpu().numpy())  # spla.norm(rmat, 2, axis=0)
    recip = np.true_divide(1.0, np.maximum(norms, np.finfo("f4").smallest_normal))
    d_recip = torch.from_numpy(np.ascontiguousarray(recip, dtype=np.float32)).to(dev)
    v_items = torch.empty(nnz, dtype=torch.float32, device=dev)
    v_users = torch.empty(nnz, dtype=torch.float32, device=dev)
    check(
        lib.lk_iknn_prep_scale(_ptr(t.indptr), is64, _ptr(t.perm), _ptr(cent), _ptr(d_recip),
                               n_items, _ptr(v_items), _ptr(v_users), _stream()),
        "lk_iknn_prep_scale",
    )
    all_zero = explicit and int(flag.item()) == 0
    ui = DeviceCSR(dcsr.indptr, dcsr.indices, v_users, (n_users, n_items), dcsr.h_indptr)
    iu = DeviceCSR(t.indptr, t.indices, v_items, (n_items, n_users), t_ptr)
    return ui, iu, means, all_zero


RANK_STATS_MAX_CUTOFFS = 8  # of one lk_rank_stats launch (csrc/metrics.hip)
RANK_STATS_MAX_TABLES = 4
IDEAL_GAIN_LDS_ROW = 4096  # longest truth row lk_ideal_gain sorts in LDS


def _i32_array(vals):
    arr = (ctypes.c_int32 * max(len(vals), 1))()
    for i, v in enumerate(vals):
        arr[i] = int(v)
    return arr


def rank_stats(lists: torch.Tensor, truth: DeviceCSR, cutoffs, weights: torch.Tensor | None,
               gains: bool = False, length: int | None = None):
    """
    The sufficient statistics of the ranking metrics for a batch of lists (lk_rank_stats):
    ``lists`` device int32 [B x ld] item numbers in rank order (negative entries dropped before
    ranking), ``truth`` the per-list truth CSR (int64 offsets, rows ascending; ``values`` = gains
    when ``gains``), ``cutoffs`` host integers (0 = whole list), ``weights`` device float64
    [tables x w_ld] or None.  Returns device (counts int32 [(2 + 2 C) x B], sums float64
    [C (1 + 2 T) x B]) laid out as include/lkamd.h says.
    """
    lib = _native.require_gpu()
    assert lists.dtype == torch.int32 and lists.dim() == 2 and lists.is_contiguous()
    B, ld = int(lists.shape[0]), int(lists.shape[1])
    ln = ld if length is None else int(length)
    assert truth.indptr.dtype == torch.int64 and int(truth.indptr.shape[0]) == B + 1
    C = len(cutoffs)
    T = 0 if weights is None else int(weights.shape[0])
    if weights is not None:
        assert weights.dtype == torch.float64 and weights.is_contiguous()
    dev = lists.device
    counts = torch.empty((2 + 2 * C, B), dtype=torch.int32, device=dev)
    sums = torch.empty((C * (1 + 2 * T), B), dtype=torch.float64, device=dev)
    check(
        lib.lk_rank_stats(_ptr(lists), B, ld, ln, _ptr(truth.indptr),
                          _ptr(truth.indices), _ptr(truth.values) if gains else None,
                          _i32_array(cutoffs), C, _ptr(weights), T,
                          0 if weights is None else int(weights.shape[1]), _ptr(counts),
                          _ptr(sums), _stream()),
        "lk_rank_stats",
    )
    return counts, sums


def ideal_gain(truth: DeviceCSR, combos, weights: torch.Tensor):
    """
    Graded NDCG's denominators (lk_ideal_gain): per row of ``truth`` (values = gains; needs the
    host copy of the offsets) and per ``combos`` entry (cutoff, table) the descending clipped
    gains dotted with the table.  Returns device (ideal float64 [combos x rows], count of
    non-NaN gains int32 [rows]).
    """
    lib = _native.require_gpu()
    R = int(truth.indptr.shape[0]) - 1
    dev = truth.indptr.device
    lens = np.diff(truth.h_indptr)
    long_rows = np.flatnonzero(lens > IDEAL_GAIN_LDS_ROW).astype(np.int32)
    longest = int(lens.max()) if R else 0
    d_long = torch.from_numpy(long_rows).to(dev) if len(long_rows) else None
    wb = lib.lk_ideal_gain_workspace_bytes(len(long_rows), longest)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev) if wb else None
    ideal = torch.zeros((len(combos), R), dtype=torch.float64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    assert weights.dtype == torch.float64 and weights.is_contiguous()
    check(
        lib.lk_ideal_gain(_ptr(truth.indptr), _ptr(truth.values), R, _ptr(d_long),
                          len(long_rows), longest, _ptr(ws), _i32_array([c for c, _t in combos]),
                          _i32_array([t for _c, t in combos]), len(combos), _ptr(weights),
                          int(weights.shape[0]), int(weights.shape[1]), _ptr(ideal), _ptr(count),
                          _stream()),
        "lk_ideal_gain",
    )
    return ideal, count


def predict_errors(pred_ptr: torch.Tensor, pred_items: torch.Tensor | None,
                   pred_scores: torch.Tensor, truth: DeviceCSR | None,
                   pred_ratings: torch.Tensor | None = None):
    """
    Squared / absolute prediction errors per list (lk_predict_errors): ragged lists (int64
    offsets, int32 item numbers, f32 scores) against the per-list ``truth`` CSR (values =
    ratings), or against ``pred_ratings`` when ``truth`` is None.  Returns device (sums float64
    [2 x B]: sse, sae; counts int32 [3 x B]: n, n_missing_score, n_missing_truth).
    """
    lib = _native.require_gpu()
    B = int(pred_ptr.shape[0]) - 1
    dev = pred_ptr.device
    assert pred_ptr.dtype == torch.int64 and pred_scores.dtype == torch.float32
    sums = torch.zeros((2, B), dtype=torch.float64, device=dev)
    counts = torch.zeros((3, B), dtype=torch.int32, device=dev)
    if truth is not None:
        assert truth.indptr.dtype == torch.int64 and int(truth.indptr.shape[0]) == B + 1
        assert pred_items is not None and pred_items.dtype == torch.int32
    else:
        assert pred_ratings is not None and pred_ratings.dtype == torch.float32
    if int(pred_scores.shape[0]) == 0:  # (no entry is read; the call wants non-null arrays)
        pred_items = torch.zeros(1, dtype=torch.int32, device=dev)
        pred_ratings = torch.zeros(1, dtype=torch.float32, device=dev)
    check(
        lib.lk_predict_errors(B, _ptr(pred_ptr), _ptr(pred_items), _ptr(pred_scores),
                              _ptr(pred_ratings), _ptr(truth.indptr) if truth else None,
                              _ptr(truth.indices) if truth else None,
                              _ptr(truth.values) if truth else None, _ptr(sums), _ptr(counts),
                              _stream()),
        "lk_predict_errors",
    )
    return sums, counts


# ---------------------------------------------------------------------------------------
# exposure / diversity / popularity / reranking metrics (csrc/diversity.hip)
# ---------------------------------------------------------------------------------------

CATEGORY_MAX = 7168  # category columns of lk_list_category_stats (lk_list_category_max())
PAIR_STATS_MAX_DEPTH = 1024  # depth n of lk_list_pair_stats


def _list_shape(lists: torch.Tensor, length):
    assert lists.dtype == torch.int32 and lists.dim() == 2 and lists.is_contiguous()
    B, ld = int(lists.shape[0]), int(lists.shape[1])
    return B, ld, ld if length is None else int(length)


def _check_table(weights, need: int):
    if weights is None:
        return 0
    assert weights.dtype == torch.float64 and weights.dim() == 1 and weights.is_contiguous()
    assert int(weights.shape[0]) >= need
    return int(weights.shape[0])


def item_exposure(lists: torch.Tensor, totals: torch.Tensor, cutoff: int = 0,
                  weights: torch.Tensor | None = None, length: int | None = None) -> None:
    """
    ``totals[item] += w(rank)`` over the kept entries of ``lists`` (lk_item_exposure): device
    int32 [B x ld] lists, float64 [n_items] ``totals`` accumulated in place, ``weights`` a device
    float64 rank table or None (every weight 1).
    """
    lib = _native.require_gpu()
    B, ld, ln = _list_shape(lists, length)
    assert totals.dtype == torch.float64 and totals.dim() == 1 and totals.is_contiguous()
    w_ld = _check_table(weights, min(ln, cutoff) if cutoff else ln)
    wb = lib.lk_item_exposure_workspace_bytes(B, ln)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=lists.device)
    check(
        lib.lk_item_exposure(_ptr(lists), B, ld, ln, int(cutoff), _ptr(weights), w_ld,
                             int(totals.shape[0]), _ptr(totals), _ptr(ws), _stream()),
        "lk_item_exposure",
    )


@dataclass
class DeviceCategories:
    "An item x category matrix in HBM: CSR with int64 offsets, int32 columns, float64 values."
    indptr: torch.Tensor
    indices: torch.Tensor
    values: torch.Tensor
    shape: tuple

    @classmethod
    def from_scipy(cls, mat, dev) -> "DeviceCategories":
        import scipy.sparse as sps

        m = sps.csr_array(mat)
        m.sum_duplicates()
        if m.shape[1] > CATEGORY_MAX:
            raise ValueError(f"{m.shape[1]} category columns: the device keeps a list's column "
                             f"sums in LDS and supports at most {CATEGORY_MAX}")
        return cls(torch.from_numpy(np.ascontiguousarray(m.indptr, dtype=np.int64)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(m.indices, dtype=np.int32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(m.data, dtype=np.float64)).to(dev),
                   tuple(m.shape))


def list_category_stats(lists: torch.Tensor, cats: DeviceCategories, cutoff: int = 0,
                        weights: torch.Tensor | None = None, length: int | None = None):
    """
    Per list the category column sums' statistics (lk_list_category_stats).  Returns device
    (known int32 [B], stats float64 [3 x B]: sq_sum, self_sum, entropy).
    """
    lib = _native.require_gpu()
    B, ld, ln = _list_shape(lists, length)
    n_items, C = int(cats.shape[0]), int(cats.shape[1])
    if C > CATEGORY_MAX:
        raise ValueError(f"{C} category columns: at most {CATEGORY_MAX} are supported")
    assert cats.indptr.dtype == torch.int64 and int(cats.indptr.shape[0]) == n_items + 1
    assert cats.indices.dtype == torch.int32 and cats.values.dtype == torch.float64
    w_ld = _check_table(weights, min(ln, cutoff) if cutoff else ln)
    known = torch.empty(B, dtype=torch.int32, device=lists.device)
    stats = torch.empty((3, B), dtype=torch.float64, device=lists.device)
    check(
        lib.lk_list_category_stats(_ptr(lists), B, ld, ln, int(cutoff), n_items,
                                   _ptr(cats.indptr), _ptr(cats.indices), _ptr(cats.values), C,
                                   _ptr(weights), w_ld, _ptr(known), _ptr(stats), _stream()),
        "lk_list_category_stats",
    )
    return known, stats


def list_gather_mean(lists: torch.Tensor, table: torch.Tensor, cutoff: int = 0,
                     length: int | None = None):
    """
    Per list the rank-order sum of ``table[item]`` (device float64 [n_items]) and the number of
    kept entries (lk_list_gather_mean).  Returns device (sum float64 [B], length int32 [B]).
    """
    lib = _native.require_gpu()
    B, ld, ln = _list_shape(lists, length)
    assert table.dtype == torch.float64 and table.dim() == 1 and table.is_contiguous()
    sums = torch.empty(B, dtype=torch.float64, device=lists.device)
    lens = torch.empty(B, dtype=torch.int32, device=lists.device)
    check(
        lib.lk_list_gather_mean(_ptr(lists), B, ld, ln, int(cutoff), _ptr(table),
                                int(table.shape[0]), _ptr(sums), _ptr(lens), _stream()),
        "lk_list_gather_mean",
    )
    return sums, lens


def list_pair_stats(a_ptr: torch.Tensor, a_items: torch.Tensor, b_ptr: torch.Tensor,
                    b_items: torch.Tensor, n: int, weights: torch.Tensor,
                    a_rows: torch.Tensor | None = None):
    """
    Rank-biased overlap's weighted agreement sum and least-item-promoted per pair of ragged lists
    (lk_list_pair_stats): reference lists ``a`` (pair ``q`` takes row ``a_rows[q]``, ``q`` itself
    without ``a_rows``), reranked lists ``b``.  Returns device (rbo_sum float64 [P], lip int32
    [P], flag int32 [P]: 1 where the reference list is empty).
    """
    lib = _native.require_gpu()
    P = int(b_ptr.shape[0]) - 1
    dev = b_ptr.device
    assert a_ptr.dtype == torch.int64 and b_ptr.dtype == torch.int64
    assert a_items.dtype == torch.int32 and b_items.dtype == torch.int32
    assert weights.dtype == torch.float64 and int(weights.shape[0]) >= n
    if a_rows is None:
        assert int(a_ptr.shape[0]) == P + 1
    else:
        assert a_rows.dtype == torch.int32 and int(a_rows.shape[0]) == P
    rbo = torch.empty(P, dtype=torch.float64, device=dev)
    lip = torch.empty(P, dtype=torch.int32, device=dev)
    flag = torch.empty(P, dtype=torch.int32, device=dev)
    check(
        lib.lk_list_pair_stats(P, _ptr(a_rows), _ptr(a_ptr), _ptr(a_items), _ptr(b_ptr),
                               _ptr(b_items), int(n), _ptr(weights), _ptr(rbo), _ptr(lip),
                               _ptr(flag), _stream()),
        "lk_list_pair_stats",
    )
    return rbo, lip, flag


def fair_rerank(lists: torch.Tensor, is_protected: torch.Tensor, m_table: torch.Tensor,
                n_out: int, *, lengths: torch.Tensor | None = None,
                scores: torch.Tensor | None = None, want_pos: bool = False):
    """
    FA*IR reranking of a batch of ranked lists (lk_fair_rerank): device int32 [B x L] ``lists``
    (rows ``stride(0)`` apart) of item numbers, ``is_protected`` uint8 [n_items], ``m_table`` int32
    (at most ``_native.FAIR_MAX_N`` entries, ``n_out`` of them used).  ``lengths``: int32 [B] or
    None (a row ends at its first negative entry); ``scores``: float32 in the layout of ``lists``,
    copied as bits.  Returns device (items int32 [B x n_out] with -1 padding, scores [B x n_out]
    with NaN padding or None, positions into the input rows or None).
    """
    lib = _native.require_gpu()
    assert lists.dtype == torch.int32 and lists.dim() == 2
    B, L = int(lists.shape[0]), int(lists.shape[1])
    assert B == 0 or L <= 1 or lists.stride(1) == 1
    ld = int(lists.stride(0)) if B > 1 and L > 0 else max(L, 1)
    assert ld >= L
    dev = lists.device
    assert is_protected.dtype == torch.uint8 and is_protected.dim() == 1 and \
        is_protected.is_contiguous()
    assert m_table.dtype == torch.int32 and m_table.dim() == 1 and m_table.is_contiguous()
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.is_contiguous()
    if scores is not None:
        assert scores.dtype == torch.float32 and scores.shape == lists.shape
        assert B == 0 or ((L <= 1 or scores.stride(1) == 1) and
                          (int(scores.stride(0)) == ld or B == 1 or L == 0))
    n_out = int(n_out)
    out = torch.empty((B, n_out), dtype=torch.int32, device=dev)
    out_sc = torch.empty((B, n_out), dtype=torch.float32, device=dev) if scores is not None \
        else None
    out_pos = torch.empty((B, n_out), dtype=torch.int32, device=dev) if want_pos else None
    check(
        lib.lk_fair_rerank(_ptr(lists), B, L, ld, _ptr(lengths), _ptr(scores), _ptr(is_protected),
                           int(is_protected.shape[0]), _ptr(m_table), int(m_table.shape[0]), n_out,
                           _ptr(out), _ptr(out_sc), _ptr(out_pos), _stream()),
        "lk_fair_rerank",
    )
    return out, out_sc, out_pos


# ---------------------------------------------------------------------------------------
# FlexMF implicit and explicit (csrc/flexmf.hip), ragged pair scoring (csrc/mf_pairs.hip)
# ---------------------------------------------------------------------------------------

_FLEXMF_TABLES = ("u_embed", "i_embed", "u_bias", "i_bias")


def _i32_dev(a, dev) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def flexmf_sample_negatives(indptr: torch.Tensor, indices: torch.Tensor, n_cols: int, rows,
                            n: int, weighting: str, key: int, counter: int = 0, *,
                            verify: bool = True, max_attempts: int = 10) -> torch.Tensor:
    """
    Negative columns for ``rows`` (lk_flexmf_sample_negatives): int32 device [len(rows) x n].
    ``indptr`` (int64) / ``indices`` (int32, ascending inside a row): the training matrix on the
    device; ``weighting``: ``uniform`` | ``popular`` | ``popularity``; the draw is a function of
    (key, counter, row position, replicate, attempt) alone.
    """
    lib = _native.require_gpu()
    if weighting not in ("uniform", "popular", "popularity"):
        raise ValueError(f"unsupported weighting {weighting}")
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32
    dev = indptr.device
    rows = _i32_dev(rows, dev)
    out = torch.empty((rows.numel(), int(n)), dtype=torch.int32, device=dev)
    check(lib.lk_flexmf_sample_negatives(
        _ptr(indptr), _ptr(indices), indices.numel(), int(n_cols), _ptr(rows), rows.numel(),
        int(n), int(weighting != "uniform"), int(bool(verify)), int(max_attempts),
        int(key) & (2**64 - 1), int(counter) & (2**64 - 1), _ptr(out), _stream()),
        "lk_flexmf_sample_negatives")
    return out


class FlexMFState:
    """
    The FlexMF model and its optimiser state in HBM: the four tables of ``FlexMFModel``
    (src/lenskit/flexmf/_model.py:73-81; an absent bias table is ``None``), Adam's two moment
    tables of each, the global step count and the step's scratch.  ``step`` is one
    ``train_batch`` + ``opt.step()`` (lk_flexmf_step) on explicit (users, positives, negatives
    [, weights]); ``warp_search`` is the misranked-negative search on an explicit candidate table.
    With ``loss="mse"`` it is the FlexMF explicit model, stepped by ``step_explicit`` (users,
    items, ratings: lk_flexmf_step_explicit).
    """

    def __init__(self, u_embed, i_embed, u_bias=None, i_bias=None, *, loss: str = "logistic",
                 reg_method: str | None = "AdamW", regularization: float = 0.01,
                 learning_rate: float = 0.01, negative_count: int = 1,
                 positive_weight: float = 1.0, dev=None):
        self.dev = dev = device(dev)
        host = [u_embed, i_embed, u_bias, i_bias]
        self.n_users, self.k = np.shape(u_embed)
        self.n_items = np.shape(i_embed)[0]
        if not 1 <= self.k <= _native.FLEXMF_MAX_K:
            raise ValueError(f"unsupported embedding size {self.k} "
                             f"(supported: 1..{_native.FLEXMF_MAX_K})")
        if np.shape(i_embed)[1] != self.k:
            raise ValueError("user and item embeddings differ in width")
        self.param, self.exp_avg, self.exp_avg_sq = [], [], []
        for i, a in enumerate(host):
            if a is None:
                t = None
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                rows = self.n_users if i in (0, 2) else self.n_items
                if i >= 2:
                    a = a.reshape(-1)
                if a.shape[0] != rows:
                    raise ValueError(f"{_FLEXMF_TABLES[i]} has {a.shape[0]} rows, not {rows}")
                t = torch.from_numpy(a).to(dev)
            self.param.append(t)
            self.exp_avg.append(None if t is None else torch.zeros_like(t))
            self.exp_avg_sq.append(None if t is None else torch.zeros_like(t))
        if loss != "mse" and loss not in _native.FLEXMF_LOSSES:
            raise ValueError(f"unknown loss {loss}")
        if reg_method not in ("AdamW", "L2", None):
            raise ValueError(f"unknown regularization method {reg_method}")
        self.loss, self.reg_method = loss, reg_method
        self.regularization, self.learning_rate = float(regularization), float(learning_rate)
        self.negative_count, self.positive_weight = int(negative_count), float(positive_weight)
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8  # the defaults of both optimisers
        self.steps = 0
        self._ws = None
        self._ws_batch = 0
        # AdamW: row -> slot of its summed gradient, all -1 between steps
        self._slot = torch.full((self.n_users + self.n_items,), -1, dtype=torch.int32,
                                device=dev) if reg_method == "AdamW" else None
        self._tables = _native.FlexMFTables()
        for i in range(4):
            self._tables.param[i] = _ptr(self.param[i]).value
            self._tables.exp_avg[i] = _ptr(self.exp_avg[i]).value
            self._tables.exp_avg_sq[i] = _ptr(self.exp_avg_sq[i]).value
        self._tables.n_users, self._tables.n_items = self.n_users, self.n_items
        self._tables.k = self.k

    def _check_indices(self, users, pos, neg):
        for name, t, bound in (("users", users, self.n_users), ("positives", pos, self.n_items),
                               ("negatives", neg, self.n_items)):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= bound):
                raise ValueError(f"{name} outside [0, {bound})")

    def step(self, users, positives, negatives, weights=None, *, loss_sum=None,
             check_indices: bool = True) -> torch.Tensor:
        "One training step; returns the batch loss (device, 1 element), nothing synchronised."
        lib = _native.require_gpu()
        dev = self.dev
        if self.loss == "mse":
            raise ValueError("a squared-error model is stepped by step_explicit")
        users, positives = _i32_dev(users, dev).reshape(-1), _i32_dev(positives, dev).reshape(-1)
        negatives = _i32_dev(negatives, dev).reshape(-1)
        B, n = users.numel(), self.negative_count
        if positives.numel() != B or negatives.numel() != B * n or B < 1:
            raise ValueError("batch arrays disagree in length")
        if self.loss == "warp":
            if weights is None or n != 1:
                raise ValueError("WARP loss takes one negative per sample and the weights")
            weights = torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
            if weights.numel() != B:
                raise ValueError("weights disagree with the batch in length")
        else:
            weights = None
        if check_indices:  # (the trainer's own arrays come from the dataset and the sampler)
            self._check_indices(users, positives, negatives)
        if self._ws is None or self._ws_batch < B:
            self._ws = torch.empty(lib.lk_flexmf_step_workspace_bytes(B, n, self.k),
                                   dtype=torch.uint8, device=dev)
            self._ws_batch = B
        self.steps += 1
        h = _native.FlexMFHyper(
            _native.FLEXMF_LOSSES[self.loss],
            _native.FLEXMF_ADAMW if self.reg_method == "AdamW" else _native.FLEXMF_SPARSE_ADAM,
            int(self.reg_method == "L2"), n, self.positive_weight, self.regularization,
            self.learning_rate, self.beta1, self.beta2, self.eps,
            1.0 - self.beta1 ** self.steps, 1.0 - self.beta2 ** self.steps)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.lk_flexmf_step(ctypes.byref(self._tables), ctypes.byref(h), _ptr(users),
                                 _ptr(positives), _ptr(negatives), _ptr(weights), B,
                                 _ptr(self._ws), _ptr(self._slot), _ptr(loss), _ptr(loss_sum),
                                 _stream()), "lk_flexmf_step")
        return loss

    def step_explicit(self, users, items, ratings, *, loss_sum=None,
                      check_indices: bool = True) -> torch.Tensor:
        """One squared-error step on (users, items, ratings); returns the batch's mean squared
        error -- without the L2 term -- (device, 1 element), nothing synchronised."""
        lib = _native.require_gpu()
        dev = self.dev
        if self.loss != "mse":
            raise ValueError(f"step_explicit needs loss 'mse', not {self.loss!r}")
        users, items = _i32_dev(users, dev).reshape(-1), _i32_dev(items, dev).reshape(-1)
        ratings = torch.as_tensor(ratings).to(device=dev, dtype=torch.float32).reshape(-1)
        ratings = ratings.contiguous()
        B = users.numel()
        if items.numel() != B or ratings.numel() != B or B < 1:
            raise ValueError("batch arrays disagree in length")
        if check_indices:
            self._check_indices(users, items, items)
        if self._ws is None or self._ws_batch < B:
            self._ws = torch.empty(lib.lk_flexmf_step_explicit_workspace_bytes(B, self.k),
                                   dtype=torch.uint8, device=dev)
            self._ws_batch = B
        self.steps += 1
        h = _native.FlexMFHyper(
            _native.FLEXMF_MSE,
            _native.FLEXMF_ADAMW if self.reg_method == "AdamW" else _native.FLEXMF_SPARSE_ADAM,
            int(self.reg_method == "L2"), 0, 1.0, self.regularization, self.learning_rate,
            self.beta1, self.beta2, self.eps, 1.0 - self.beta1 ** self.steps,
            1.0 - self.beta2 ** self.steps)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.lk_flexmf_step_explicit(ctypes.byref(self._tables), ctypes.byref(h),
                                          _ptr(users), _ptr(items), _ptr(ratings), B,
                                          _ptr(self._ws), _ptr(self._slot), _ptr(loss),
                                          _ptr(loss_sum), _stream()), "lk_flexmf_step_explicit")
        return loss

    def warp_search(self, users, positives, candidates, *, check_indices: bool = True):
        """
        The misranked-negative search over ``candidates`` [B x tries] (lk_flexmf_warp_search):
        (negatives int32 [B], counts int32 [B], weights float64 [B]) on the device.
        """
        lib = _native.require_gpu()
        dev = self.dev
        users, positives = _i32_dev(users, dev).reshape(-1), _i32_dev(positives, dev).reshape(-1)
        candidates = _i32_dev(candidates, dev)
        B = users.numel()
        if candidates.dim() != 2 or candidates.shape[0] != B or positives.numel() != B:
            raise ValueError("candidate table disagrees with the batch")
        if check_indices:
            self._check_indices(users, positives, candidates)
        neg = torch.empty(B, dtype=torch.int32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        weight = torch.empty(B, dtype=torch.float64, device=dev)
        check(lib.lk_flexmf_warp_search(ctypes.byref(self._tables), _ptr(users), _ptr(positives),
                                        _ptr(candidates), B, candidates.shape[1], _ptr(neg),
                                        _ptr(count), _ptr(weight), _stream()),
              "lk_flexmf_warp_search")
        return neg, count, weight

    def host_tables(self) -> dict:
        "The four parameter tables as host arrays under Torch's ``state_dict`` names."
        return {f"{name}.weight": None if t is None else
                (t.cpu().numpy() if i < 2 else t.cpu().numpy().reshape(-1, 1))
                for i, (name, t) in enumerate(zip(_FLEXMF_TABLES, self.param))}

    def load_tables(self, state) -> None:
        for name, t in zip(_FLEXMF_TABLES, self.param):
            val = state.get(f"{name}.weight")
            if t is not None and val is not None:
                val = torch.as_tensor(np.asarray(val, dtype=np.float32)).reshape(t.shape)
                t.copy_(val.to(self.dev))


def flexmf_gather_batch(perm: torch.Tensor, all_users: torch.Tensor, all_items: torch.Tensor):
    "(users, items) of one batch: ``all[perm]`` of both arrays (lk_flexmf_gather_batch)."
    lib = _native.require_gpu()
    assert perm.dtype == torch.int32 and perm.is_contiguous()
    n = perm.numel()
    users = torch.empty(n, dtype=torch.int32, device=perm.device)
    items = torch.empty(n, dtype=torch.int32, device=perm.device)
    check(lib.lk_flexmf_gather_batch(_ptr(perm), n, _ptr(all_users), _ptr(all_items),
                                     _ptr(users), _ptr(items), _stream()),
          "lk_flexmf_gather_batch")
    return users, items


def flexmf_gather_values(perm: torch.Tensor, all_values: torch.Tensor) -> torch.Tensor:
    "``all_values[perm]`` of a float32 array, the ratings of one batch (lk_flexmf_gather_values)."
    lib = _native.require_gpu()
    assert perm.dtype == torch.int32 and perm.is_contiguous()
    assert all_values.dtype == torch.float32 and all_values.is_contiguous()
    out = torch.empty(perm.numel(), dtype=torch.float32, device=perm.device)
    check(lib.lk_flexmf_gather_values(_ptr(perm), perm.numel(), _ptr(all_values), _ptr(out),
                                      _stream()), "lk_flexmf_gather_values")
    return out


def mf_score_pairs(users: torch.Tensor, items: torch.Tensor, k: int, user_rows: torch.Tensor,
                   tgt_ptr: torch.Tensor, tgt_items: torch.Tensor) -> torch.Tensor:
    """
    Ragged pair scores (lk_mf_score_pairs): ``users`` [U x KP] / ``items`` [I x KP] padded device
    operands of inner width ``k``; query q is row ``user_rows[q]`` (int32) against the items
    ``tgt_items[tgt_ptr[q]:tgt_ptr[q + 1]]`` (int64 offsets from 0, int32 items).  Returns f32
    [len(tgt_items)] on the device, NaN where the user row or the item is -1.
    """
    lib = _native.require_gpu()
    assert users.dtype == torch.float32 and users.is_contiguous() and users.dim() == 2
    assert items.dtype == torch.float32 and items.is_contiguous() and items.dim() == 2
    assert user_rows.dtype == torch.int32 and tgt_items.dtype == torch.int32
    assert tgt_ptr.dtype == torch.int64 and tgt_ptr.numel() == user_rows.numel() + 1
    assert user_rows.is_contiguous() and tgt_ptr.is_contiguous() and tgt_items.is_contiguous()
    out = torch.empty(tgt_items.numel(), dtype=torch.float32, device=users.device)
    check(lib.lk_mf_score_pairs(_ptr(users), users.shape[1], users.shape[0], _ptr(items),
                                items.shape[1], items.shape[0], int(k), _ptr(user_rows),
                                user_rows.numel(), _ptr(tgt_ptr), _ptr(tgt_items),
                                tgt_items.numel(), _ptr(out), _stream()), "lk_mf_score_pairs")
    return out


# ---- per-query candidate lists (csrc/candidates.hip) ----------------------------------------
def check_ragged(h_tgt_ptr, n_queries: int, total: int) -> np.ndarray:
    """
    The host copy of a batch's target offsets, validated before anything is launched: int64, one
    per query and one more, ascending from 0 to ``total``.  Raises ``ValueError`` otherwise.
    """
    ptr = np.ascontiguousarray(h_tgt_ptr, dtype=np.int64).reshape(-1)
    if len(ptr) != n_queries + 1 or ptr[0] != 0 or ptr[-1] != total or (np.diff(ptr) < 0).any():
        raise ValueError("tgt_ptr must ascend from 0 to len(tgt_items), one entry per query and "
                         "one more")
    return ptr


def upload_targets(h_tgt_ptr: np.ndarray, item_nums: np.ndarray, dev):
    """
    The ragged targets of a batch in ONE upload: (device int64 offsets [B + 1], device int32 item
    numbers [total]), views of one packed tensor.  ``h_tgt_ptr`` is validated first.
    """
    item_nums = np.ascontiguousarray(item_nums, dtype=np.int32).reshape(-1)
    n = len(item_nums)
    ptr = check_ragged(h_tgt_ptr, len(np.reshape(h_tgt_ptr, -1)) - 1, n)
    head = 2 * len(ptr)
    packed = np.empty(head + n, np.int32)
    packed[:head] = ptr.view(np.int32)
    packed[head:] = item_nums
    d_packed = torch.from_numpy(packed).to(dev)
    return d_packed[:head].view(torch.int64), d_packed[head:]


def _ragged_args(h_tgt_ptr, tgt_ptr: torch.Tensor, tgt_items: torch.Tensor) -> np.ndarray:
    assert tgt_ptr.dtype == torch.int64 and tgt_ptr.is_contiguous() and tgt_ptr.dim() == 1
    assert tgt_items.dtype == torch.int32 and tgt_items.is_contiguous() and tgt_items.dim() == 1
    if tgt_items.numel() >= 2 ** 31:
        raise ValueError("more than 2^31 targets in one call")
    return check_ragged(h_tgt_ptr, tgt_ptr.numel() - 1, tgt_items.numel())


def score_candidates(users: torch.Tensor, items: torch.Tensor, k: int, user_rows: torch.Tensor,
                     tgt_ptr: torch.Tensor, tgt_items: torch.Tensor, h_tgt_ptr) -> torch.Tensor:
    """
    Ragged pair scores as the k-ordered chain of :func:`score_dense` (lk_score_candidates): the
    arguments of :func:`mf_score_pairs` plus ``h_tgt_ptr``, the host copy of the offsets, which is
    validated before the launch.  Returns f32 [len(tgt_items)] on the device: entry t has the bits
    of ``score_dense(users, items, k)[user_rows[q], tgt_items[t]]``, NaN where the user row or the
    item is outside its table.
    """
    lib = _native.require_gpu()
    assert users.dtype == torch.float32 and users.is_contiguous() and users.dim() == 2
    assert items.dtype == torch.float32 and items.is_contiguous() and items.dim() == 2
    assert user_rows.dtype == torch.int32 and user_rows.is_contiguous()
    assert tgt_ptr.numel() == user_rows.numel() + 1
    _ragged_args(h_tgt_ptr, tgt_ptr, tgt_items)
    out = torch.empty(tgt_items.numel(), dtype=torch.float32, device=users.device)
    check(lib.lk_score_candidates(_ptr(users), users.shape[1], users.shape[0], _ptr(items),
                                  items.shape[1], items.shape[0], int(k), _ptr(user_rows),
                                  user_rows.numel(), _ptr(tgt_ptr), _ptr(tgt_items),
                                  tgt_items.numel(), _ptr(out), _stream()), "lk_score_candidates")
    return out


def panel_take_ragged(panel: torch.Tensor, n_items: int, tgt_ptr: torch.Tensor,
                      tgt_items: torch.Tensor, h_tgt_ptr) -> torch.Tensor:
    """
    ``panel[q, tgt_items[t]]`` for every t of query q's range (lk_panel_take_ragged): ``panel`` a
    device f32 [queries x ld] score panel of which ``n_items`` columns are items.  Returns f32
    [len(tgt_items)] on the device, NaN for an item outside ``[0, n_items)``.
    """
    lib = _native.require_gpu()
    assert panel.dtype == torch.float32 and panel.dim() == 2 and panel.stride(1) == 1
    assert panel.shape[0] == tgt_ptr.numel() - 1 and panel.shape[1] >= n_items
    _ragged_args(h_tgt_ptr, tgt_ptr, tgt_items)
    out = torch.empty(tgt_items.numel(), dtype=torch.float32, device=panel.device)
    check(lib.lk_panel_take_ragged(_ptr(panel), panel.shape[0], int(n_items), panel.stride(0),
                                   _ptr(tgt_ptr), _ptr(tgt_items), tgt_items.numel(), _ptr(out),
                                   _stream()), "lk_panel_take_ragged")
    return out


def sparse_score_candidates(hist: DeviceCSR, model: DeviceCSR, reduce: str,
                            tgt_ptr: torch.Tensor, tgt_items: torch.Tensor, h_tgt_ptr, *,
                            rows: torch.Tensor | None = None) -> torch.Tensor:
    """
    The entries of the :func:`slim_score_batch` (``reduce="sum"``) or :func:`assoc_score_batch`
    (``"mean"``, ``"max"``) panel at ragged targets, without the panel
    (lk_sparse_score_candidates): per target a chain over the query's history rows of the sparse
    ``model`` (int64 offsets, columns ascending inside a row), in history order.  ``hist``: the
    histories (int64 offsets, -1 = unknown item); query q reads row ``rows[q]`` (device int32,
    outside the CSR -- -1 -- = no history) or, without ``rows``, row q.  Returns f32
    [len(tgt_items)] on the device: NaN for a target outside the model's columns, for a query
    without history (``"sum"``) / without a known history item (``"mean"``, ``"max"``).
    """
    lib = _native.require_gpu()
    if reduce not in _native.SPARSE_REDUCTIONS:
        raise ValueError(f"sparse_score_candidates: unknown reduction {reduce!r}")
    n = int(model.shape[1])
    assert model.shape[0] == n and model.indptr.dtype == torch.int64
    assert model.indptr.numel() == n + 1 and model.indices.dtype == torch.int32
    assert model.values is not None and model.values.dtype == torch.float32
    assert model.values.numel() == model.indices.numel()
    assert hist.indptr.dtype == torch.int64 and hist.indices.dtype == torch.int32
    n_hist = int(hist.indptr.numel()) - 1
    nq = tgt_ptr.numel() - 1
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.shape == (nq,)
    else:
        assert n_hist >= nq
    _ragged_args(h_tgt_ptr, tgt_ptr, tgt_items)
    out = torch.empty(tgt_items.numel(), dtype=torch.float32, device=model.indices.device)
    check(lib.lk_sparse_score_candidates(
        _ptr(hist.indptr), _ptr(hist.indices), n_hist, hist.nnz, _ptr(rows), nq,
        _ptr(model.indptr), _ptr(model.indices), _ptr(model.values), n, model.nnz,
        _ptr(tgt_ptr), _ptr(tgt_items), tgt_items.numel(), _native.SPARSE_REDUCTIONS[reduce],
        _ptr(out), _stream()), "lk_sparse_score_candidates")
    return out


def ragged_topn_classes() -> tuple[int, int]:
    """The longest segment :func:`ragged_topn` ranks in one wave, and in one workgroup
    (lk_ragged_topn_wave_max, lk_ragged_topn_block_max); longer ones are sorted."""
    lib = _native.load()
    return int(lib.lk_ragged_topn_wave_max()), int(lib.lk_ragged_topn_block_max())


def ragged_topn(tgt_ptr: torch.Tensor, tgt_items: torch.Tensor, scores: torch.Tensor, n: int,
                h_tgt_ptr):
    """
    :func:`argtopn` per segment of ragged scores (lk_ragged_topn): (item numbers int32
    [queries x width] padded with -1, scores f32 [queries x width] padded with NaN) on the
    device, ``width = n`` or, with ``n < 0``, the longest segment.  NaN scores and negative item
    numbers are dropped; ties go to the lower position; the scores are the input's own bits.
    """
    lib = _native.require_gpu()
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    assert scores.numel() == tgt_items.numel()
    ptr = _ragged_args(h_tgt_ptr, tgt_ptr, tgt_items)
    nq, total = len(ptr) - 1, tgt_items.numel()
    max_len = int(np.diff(ptr).max()) if nq else 0
    n = int(n)
    width = max_len if n < 0 else n
    idx = torch.empty((nq, width), dtype=torch.int32, device=scores.device)
    out = torch.empty((nq, width), dtype=torch.float32, device=scores.device)
    if nq == 0 or width == 0:
        return idx, out
    wb = lib.lk_ragged_topn_workspace_bytes(total, max_len)
    ws = torch.empty(wb, dtype=torch.uint8, device=scores.device) if wb else None
    check(lib.lk_ragged_topn(nq, _ptr(tgt_ptr), _ptr(tgt_items), _ptr(scores), total,
                             n if n >= 0 else -1, max_len, _ptr(ws), _ptr(idx), _ptr(out),
                             _stream()), "lk_ragged_topn")
    return idx, out


def ragged_stochastic_chunk() -> int:
    """The entries :func:`ragged_stochastic_keys` stages per wave (lk_ragged_stochastic_chunk): a
    longer segment is walked in chunks of that many."""
    return int(_native.load().lk_ragged_stochastic_chunk())


def check_ragged_addresses(h_ptr, h_addr, h_widths):
    """
    The host copies of a ragged key call, validated before anything is launched: offsets as
    :func:`check_ragged` takes them, int32 addresses that ascend strictly inside a segment and lie
    in ``[0, width of the segment)``, one int32 width per segment.  Raises ``ValueError``
    otherwise.  Returns the three as contiguous arrays.
    """
    addr = np.ascontiguousarray(h_addr, dtype=np.int32).reshape(-1)
    widths = np.ascontiguousarray(h_widths, dtype=np.int32).reshape(-1)
    if len(addr) >= 2 ** 31:
        raise ValueError("more than 2^31 entries in one call")
    ptr = check_ragged(h_ptr, len(widths), len(addr))
    if len(addr):
        lens = np.diff(ptr)
        if (addr < 0).any() or (addr >= np.repeat(widths, lens)).any():
            raise ValueError("addresses must lie in [0, width) of their segment")
        inner = np.ones(len(addr), np.bool_)
        inner[ptr[:-1][lens > 0]] = False  # (a segment's first entry has no predecessor)
        if (np.diff(addr, prepend=addr[:1])[inner] <= 0).any():
            raise ValueError("addresses must ascend strictly inside a segment")
    return ptr, addr, widths


def ragged_stochastic_keys(h_ptr, h_addr, scores, h_widths, streams, *, transform, scale: float,
                           seed: int, samples: int = 1, first_sample: int = 0):
    """
    The stochastic ranker's keys for ragged candidate lists (lk_ragged_stochastic_keys): segment
    s -- the entries ``h_ptr[s]:h_ptr[s + 1]`` -- stands for the row of a [1 x ``h_widths[s]``]
    panel with ``scores[t]`` (device f32 [total], or a host array) at column ``h_addr[t]`` and NaN
    elsewhere, and gets the bits :func:`stochastic_keys` gives that row under stream
    ``streams[s]`` -- without the row.  The host arrays are validated
    (:func:`check_ragged_addresses`) and go up in ONE packed transfer.  Returns (keys f32
    [samples x total], sample ``first_sample + j`` in row j, NaN for an entry with a non-finite
    score; stats f32 [segments x 4]; the device offsets int64; the device addresses int32).
    """
    ptr, addr, widths = check_ragged_addresses(h_ptr, h_addr, h_widths)
    code = _native.STOCHASTIC_TRANSFORMS[transform]
    samples = int(samples)
    if samples < 0 or first_sample < 0 or first_sample + samples > 2 ** 32:
        raise ValueError("samples must be addressable by 32 bits")
    lib = _native.require_gpu()
    B, total = len(widths), len(addr)
    if isinstance(scores, torch.Tensor):
        dev = scores.device
    else:
        dev = device()
        scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(dev)
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (total,)
    head = 2 * (B + 1)
    packed = np.empty(head + total + B, np.int32)
    packed[:head] = ptr.view(np.int32)
    packed[head:head + total] = addr
    packed[head + total:] = widths
    d_packed = torch.from_numpy(packed).to(dev)
    d_ptr = d_packed[:head].view(torch.int64)
    d_addr, d_widths = d_packed[head:head + total], d_packed[head + total:]
    keys = torch.empty((samples, total), dtype=torch.float32, device=dev)
    stats = torch.empty((B, 4), dtype=torch.float32, device=dev)
    if B:
        check(lib.lk_ragged_stochastic_keys(
            B, _ptr(d_ptr), _ptr(d_addr), _ptr(scores), total, _ptr(d_widths),
            _ptr(_row_streams(streams, B, dev)), code, float(scale), int(seed) & (2**64 - 1),
            int(first_sample), samples, _ptr(stats), _ptr(keys), _stream()),
            "lk_ragged_stochastic_keys")
    return keys, stats, d_ptr, d_addr


def bmf_finish_ragged(dots: torch.Tensor, mode: torch.Tensor, ub: torch.Tensor,
                      global_bias: float, item_biases: torch.Tensor, tgt_ptr: torch.Tensor,
                      tgt_items: torch.Tensor, h_tgt_ptr) -> torch.Tensor:
    """
    ``BiasedMFScorer.finalize_scores`` in place on ragged dot products (lk_bmf_finish_ragged):
    ``dots`` f32 [total] is what :func:`score_candidates` returns for the rows whose lists are
    ``tgt_ptr`` / ``tgt_items``; per row a mode (uint8, ``_native.BMF_*``) and a float64 user
    bias.  The arithmetic is :func:`bmf_finish_pairs`'s; an unknown item (-1) is NaN.  Returns
    ``dots``.
    """
    lib = _native.require_gpu()
    rows = tgt_ptr.numel() - 1
    assert dots.dtype == torch.float32 and dots.is_contiguous()
    assert dots.numel() == tgt_items.numel()
    assert mode.dtype == torch.uint8 and mode.shape == (rows,) and mode.is_contiguous()
    assert ub.dtype == torch.float64 and ub.shape == (rows,) and ub.is_contiguous()
    assert item_biases.dtype == torch.float32 and item_biases.is_contiguous()
    _ragged_args(h_tgt_ptr, tgt_ptr, tgt_items)
    check(lib.lk_bmf_finish_ragged(_ptr(dots), rows, int(item_biases.shape[0]), _ptr(mode),
                                   _ptr(ub), float(global_bias), _ptr(item_biases),
                                   _ptr(tgt_ptr), _ptr(tgt_items), dots.numel(), _ptr(dots),
                                   _stream()), "lk_bmf_finish_ragged")
    return dots


# ---- randomized truncated SVD (csrc/svd.hip) ------------------------------------------------
SVD_OVERSAMPLES = 10  # sklearn's ``n_oversamples`` default, which ``TruncatedSVD`` passes on


def spmm_split() -> int:
    "The entries of one chain segment of ``lk_csr_spmm`` (lk_spmm_split): longer rows are cut."
    return int(_native.load().lk_spmm_split())


def chol_max_l() -> int:
    "The largest Gramian ``lk_chol_upper_inverse`` factors in LDS (lk_chol_max_l)."
    return int(_native.load().lk_chol_max_l())


def csr_spmm(csr: DeviceCSR, x: torch.Tensor, l: int) -> torch.Tensor:
    """
    Sparse x tall-skinny (lk_csr_spmm): ``csr`` [rows x cols] times the padded panel ``x``
    [cols x LD] (``l`` columns in use) -> a padded panel [rows x LD], pad columns zero.
    """
    lib = _native.require_gpu()
    n_rows, n_cols = csr.shape
    ld = padded_dim(l)
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (n_cols, ld)
    assert csr.values is not None and csr.values.dtype == torch.float32
    out = torch.empty((n_rows, ld), dtype=torch.float32, device=x.device)
    check(
        lib.lk_csr_spmm(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                        _ptr(csr.values), n_rows, n_cols, csr.nnz, _ptr(x), ld, int(l),
                        _ptr(out), ld, _stream()),
        "lk_csr_spmm",
    )
    return out


def chol_upper_inverse(gram: torch.Tensor, flag: torch.Tensor, step: int, *,
                       want_lower: bool = False):
    """
    ``gram`` [l x l] = R^T R -> ((R^-1)^T, R^T | None), each [LD x LD] lower triangular with
    zeros elsewhere (LD = the padded width of l): ``lk_chol_upper_inverse`` up to
    :func:`chol_max_l`, the library's ``cholesky_ex`` + ``solve_triangular`` beyond it.  A pivot
    that is not positive stores ``step`` into ``flag`` (device int32 [1]) if that is still 0;
    nothing is read back here.
    """
    lib = _native.require_gpu()
    l = int(gram.shape[0])
    ld = padded_dim(l)
    dev = gram.device
    assert gram.dtype == torch.float32 and gram.shape[1] == l and gram.stride(1) == 1
    assert flag.dtype == torch.int32 and flag.numel() == 1 and int(step) != 0
    if l <= chol_max_l():
        inv = torch.empty((ld, ld), dtype=torch.float32, device=dev)
        lower = torch.empty((ld, ld), dtype=torch.float32, device=dev) if want_lower else None
        check(lib.lk_chol_upper_inverse(_ptr(gram), gram.stride(0), l, _ptr(lower), _ptr(inv), ld,
                                        _ptr(flag), int(step), _stream()),
              "lk_chol_upper_inverse")
        return inv, lower
    # float64 inside, as the kernel carries its sums: the float32 factors are rounded once
    low, info = torch.linalg.cholesky_ex(gram.double())
    bad = (info != 0) | ~torch.isfinite(low).all()
    flag.copy_(torch.where((flag == 0) & bad, torch.full_like(flag, int(step)), flag))
    eye = torch.eye(l, dtype=torch.float64, device=dev)
    low = torch.where(bad, eye, low).float()
    inv = torch.zeros((ld, ld), dtype=torch.float32, device=dev)
    inv[:l, :l] = torch.linalg.solve_triangular(low.double(), eye, upper=False).float()
    lower = None
    if want_lower:
        lower = torch.zeros((ld, ld), dtype=torch.float32, device=dev)
        lower[:l, :l] = low
    return inv, lower


class CholeskyQR2:
    """
    ``orth``: the orthonormal basis of a padded panel's columns by CholeskyQR2 -- Gramian
    (lk_gramian), the inverse of its Cholesky factor (lk_chol_upper_inverse), the panel times
    that (lk_score_dense), and the same again on the result, which repairs the first pass's loss
    of orthogonality.  Everything is queued on the current stream; a Gramian that is not positive
    definite records its step in ``flag``, which :meth:`failed_step` reads (a synchronisation).
    """

    def __init__(self, l: int, dev):
        self.l, self.ld, self.dev = int(l), padded_dim(l), dev
        self.gramian = Gramian(self.l, dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps: list[str] = []

    def __call__(self, y: torch.Tensor, what: str, keep_factor: bool = False):
        "Q [rows x LD]; with ``keep_factor`` also R^T = L1 L2 ... as (Q, R^T [LD x LD])"
        lowers = []
        for p in (1, 2):
            self.steps.append(f"{what}, CholeskyQR pass {p}")
            inv, low = chol_upper_inverse(self.gramian(y, 0.0), self.flag, len(self.steps),
                                          want_lower=keep_factor)
            y = score_dense(y, inv, self.l)  # Y R^-1: rows of ``inv`` beyond l are zero pads
            lowers.append(low)
        if not keep_factor:
            return y
        # R = R2 R1, so R^T = L1 L2 with L = R^T: (L1 L2)[i][j] = L1[i] . (L2^T)[j]
        return y, score_dense(lowers[0], lowers[1].t().contiguous(), self.l)

    def failed_step(self) -> str | None:
        step = int(self.flag.item())
        return None if step == 0 else self.steps[step - 1]


def randomized_svd(csr: DeviceCSR, csr_t: DeviceCSR, k: int, n_iter: int, omega: np.ndarray, *,
                   device_output: bool = False, stats: dict | None = None):
    """
    Randomized truncated SVD of the sparse matrix ``csr`` (``csr_t``: its transpose,
    :func:`csr_transpose`), following sklearn's ``randomized_svd`` / ``randomized_range_finder``
    as ``TruncatedSVD.fit_transform`` calls them, step for step: ``l = k + 10`` sketch columns
    from the Gaussian start panel ``omega`` [min(shape) x l]; the transpose is operated on when
    there are fewer rows than columns; ``n_iter`` rounds of ``Q <- orth(M Q); Q <- orth(M^T Q)``
    and a last ``Q <- orth(M Q)``; ``B^T = M^T Q = Q_b R_b``; the float64 SVD of the l x l
    ``R_b`` on the host (the only host arithmetic); truncation to ``k``;
    ``svd_flip(u_based_decision=False)``; ``transformed = A components^T``.  ``orth`` is
    :class:`CholeskyQR2` where sklearn normalises by LU and QR: the result depends on the range of
    the sketch only.

    Returns (singular_values float64 [k], components f32 [k x n_cols], transformed f32
    [n_rows x k]) on the host; with ``device_output`` the last two stay on the device as padded
    panels: item factors [n_cols x KP] (= components^T) and transformed [n_rows x KP].

    ``ValueError`` unless ``k + 10 <= min(shape)`` and ``k + 10 <= 1024``; ``RuntimeError``
    naming the step when a sketch is numerically rank-deficient (never NaN factors).

    ``stats`` (a dict, for the timing tool): the stream is synchronised around every step and the
    dict receives the seconds spent in ``spmm`` and ``orth`` and the number of ``spmm_calls``.
    """
    import scipy.linalg as sla
    from time import perf_counter

    n_rows, n_cols = csr.shape
    k, n_iter = int(k), int(n_iter)
    l = k + SVD_OVERSAMPLES
    if k < 1 or l > min(n_rows, n_cols):
        raise ValueError(f"randomized_svd: k + {SVD_OVERSAMPLES} = {l} sketch columns need a "
                         f"matrix of at least that many rows and columns, got {csr.shape}")
    if l > 1024:
        raise ValueError(f"randomized_svd: k + {SVD_OVERSAMPLES} = {l} exceeds 1024")
    if tuple(csr_t.shape) != (n_cols, n_rows) or csr_t.nnz != csr.nnz:
        raise ValueError("randomized_svd: csr_t is not the transpose of csr")
    transpose = n_rows < n_cols  # sklearn's transpose="auto"
    m, mt = (csr_t, csr) if transpose else (csr, csr_t)
    omega = np.asarray(omega, dtype=np.float32)
    if omega.shape != (m.shape[1], l):
        raise ValueError(f"randomized_svd: omega must be {(m.shape[1], l)}, got {omega.shape}")
    dev = csr.indices.device
    orth = CholeskyQR2(l, dev)
    spmm = csr_spmm
    if stats is not None:
        stats.update(spmm=0.0, orth=0.0, spmm_calls=0)

        def timed(fn, key):
            def run(*a, **kw):
                torch.cuda.synchronize(dev)
                t0 = perf_counter()
                out = fn(*a, **kw)
                torch.cuda.synchronize(dev)
                stats[key] += perf_counter() - t0
                stats[key + "_calls"] = stats.get(key + "_calls", 0) + 1
                return out
            return run

        spmm, orth_call = timed(csr_spmm, "spmm"), timed(orth.__call__, "orth")
    else:
        orth_call = orth.__call__

    def fail(step):
        raise RuntimeError(f"randomized_svd: the sketch is numerically rank-deficient (its "
                           f"Gramian has no Cholesky factor) at: {step}")

    q = to_device_padded(omega, dev)
    for it in range(1, n_iter + 1):
        q = orth_call(spmm(m, q, l), f"power iteration {it}, M Q")
        q = orth_call(spmm(mt, q, l), f"power iteration {it}, M^T Q")
    q = orth_call(spmm(m, q, l), "range basis, M Q")
    q_b, rbt = orth_call(spmm(mt, q, l), "B^T = M^T Q", keep_factor=True)
    r_b = rbt[:l, :l].cpu().numpy().T.astype(np.float64)  # the one download inside the fit
    if not np.isfinite(r_b).all():
        fail(orth.failed_step() or "B^T = M^T Q")
    w, s, zt = sla.svd(r_b, lapack_driver="gesdd")
    # B = Z S (Q_b W)^T: M's left vectors are Q Z, its right vectors Q_b W; A's right vectors
    # are the left ones of M = A^T
    basis, rot = (q, zt.T[:, :k]) if transpose else (q_b, w[:, :k])
    kp = padded_dim(k)
    rot_t = np.zeros((kp, l), dtype=np.float32)  # the "items" operand: rows beyond k are pads
    rot_t[:k] = rot.T
    v = score_dense(basis, to_device_padded(rot_t, dev), l)  # [n_cols x KP]
    # svd_flip(u_based_decision=False): a component's largest-magnitude entry is made positive
    top = v.abs().argmax(dim=0, keepdim=True)
    sign = torch.where(v.gather(0, top) < 0, -1.0, 1.0).to(torch.float32)
    v = (v * sign).contiguous()
    transformed = spmm(csr, v, k)
    step = orth.failed_step()  # the synchronisation at the end
    if step is not None:
        fail(step)
    if device_output:
        return s[:k], v, transformed
    return s[:k], np.ascontiguousarray(to_host_unpadded(v, k).T), to_host_unpadded(transformed, k)


# ---- LightGCN (csrc/lightgcn.hip) --------------------------------------------------------------
def lgcn_ld(k: int) -> int:
    "The leading dimension of a LightGCN panel: ``k`` rounded up to whole float4 chunks."
    return (int(k) + 3) // 4 * 4


def lgcn_panel(mat: np.ndarray, dev) -> torch.Tensor:
    "Host [n x k] float32 -> device [n x lgcn_ld(k)] with zero pad columns."
    mat = np.ascontiguousarray(mat, dtype=np.float32)
    n, k = mat.shape
    out = torch.zeros((n, lgcn_ld(k)), dtype=torch.float32, device=dev)
    out[:, :k] = torch.from_numpy(mat).to(dev)
    return out


def lgcn_propagate(indptr: torch.Tensor, indices: torch.Tensor, scale: torch.Tensor, a: float,
                   x: torch.Tensor | None, b: float, t: torch.Tensor, k: int,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """
    ``out[r] = a x[r] + b scale[r] sum_e scale[col_e] t[col_e]`` over the entries of CSR row r
    (lk_lgcn_propagate): ``indptr`` int64 [n + 1], ``indices`` int32, ``scale`` float32 [n],
    ``x`` (or None: no ``a x`` term) and ``t`` padded panels [n x lgcn_ld(k)].
    """
    lib = _native.require_gpu()
    n, ld = t.shape
    assert indptr.dtype == torch.int64 and indptr.numel() == n + 1 and indptr.is_contiguous()
    assert indices.dtype == torch.int32 and indices.is_contiguous()
    assert scale.dtype == torch.float32 and scale.numel() == n and scale.is_contiguous()
    for p in (x, t, out):
        assert p is None or (p.dtype == torch.float32 and p.is_contiguous()
                             and tuple(p.shape) == (n, ld))
    if out is None:
        out = torch.empty_like(t)
    check(lib.lk_lgcn_propagate(_ptr(indptr), _ptr(indices), _ptr(scale), n, indices.numel(),
                                float(a), _ptr(x), float(b), _ptr(t), int(k), ld, _ptr(out),
                                _stream()), "lk_lgcn_propagate")
    return out


def adamw_dense(param: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                grad: torch.Tensor, k: int, *, step: int, learning_rate: float,
                weight_decay: float, beta1: float = 0.9, beta2: float = 0.999,
                eps: float = 1e-8) -> None:
    "Step ``step`` (from 1) of ``torch.optim.AdamW`` on one padded panel, in place (lk_adamw_dense)."
    lib = _native.require_gpu()
    n, ld = param.shape
    for p in (param, exp_avg, exp_avg_sq, grad):
        assert p.dtype == torch.float32 and p.is_contiguous() and tuple(p.shape) == (n, ld)
    check(lib.lk_adamw_dense(_ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(grad), n, int(k),
                             ld, float(learning_rate), float(weight_decay), float(beta1),
                             float(beta2), float(eps), 1.0 - beta1 ** step, 1.0 - beta2 ** step,
                             _stream()), "lk_adamw_dense")


class LightGCNState:
    """
    The LightGCN model and its optimiser state in HBM: the embedding panel ``X`` [n x LD] of the
    n = items + users nodes (items first), AdamW's two moment panels, the adjacency ``M`` (CSR:
    ``indptr`` int64, ``indices`` int32) with ``scale`` = degree^-1/2, three work panels and the
    pair gradient's scratch.  ``blend``: the L + 1 layer weights alpha_0 .. alpha_L.

    ``step`` is one batch: forward by L ``lk_lgcn_propagate`` launches (Horner form:
    ``t_L = alpha_L x``, ``t_j = alpha_j x + Mhat t_{j+1}``), ``lk_lgcn_pair_grad``, backward by
    the same L launches on the gradient panel, ``lk_adamw_dense``.
    """

    def __init__(self, embeddings, indptr, indices, scale, blend, *, loss: str = "pairwise",
                 regularization: float | None = 0.01, learning_rate: float = 0.01, dev=None):
        self.dev = dev = device(dev)
        self.n, self.k = np.shape(embeddings)
        if not 1 <= self.k <= _native.FLEXMF_MAX_K:
            raise ValueError(f"unsupported embedding size {self.k} "
                             f"(supported: 1..{_native.FLEXMF_MAX_K})")
        if loss not in ("pairwise", "logistic"):
            raise ValueError(f"unknown loss {loss}")
        self.blend = [float(a) for a in blend]
        if len(self.blend) < 2:
            raise ValueError("LightGCN needs at least one layer (two blend weights)")
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        scale = np.ascontiguousarray(scale, dtype=np.float32)
        if len(indptr) != self.n + 1 or len(scale) != self.n or indptr[0] != 0 or \
                indptr[-1] != len(indices) or (np.diff(indptr) < 0).any():
            raise ValueError("the adjacency does not describe the embedding table's nodes")
        if len(indices) and (indices.min() < 0 or indices.max() >= self.n):
            raise ValueError(f"adjacency columns outside [0, {self.n})")
        self.indptr = torch.from_numpy(indptr).to(dev)
        self.indices = torch.from_numpy(indices).to(dev)
        self.scale = torch.from_numpy(scale).to(dev)
        self.X = lgcn_panel(embeddings, dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.X), torch.zeros_like(self.X)
        self._work = [torch.empty_like(self.X) for _ in range(3)]  # two running panels, g
        self.loss = loss
        self.weight_decay = 0.0 if regularization is None else float(regularization)
        self.learning_rate = float(learning_rate)
        self.steps = 0
        self._ws = None
        self._ws_batch = 0

    @property
    def layers(self) -> int:
        return len(self.blend) - 1

    def propagate(self, x: torch.Tensor) -> torch.Tensor:
        "sum_l alpha_l Mhat^l x in Horner form; the result is one of the two running panels"
        al = self.blend
        L = self.layers
        out, other = self._work[0], self._work[1]
        lgcn_propagate(self.indptr, self.indices, self.scale, al[L - 1], x, al[L], x, self.k, out)
        for j in range(L - 2, -1, -1):
            lgcn_propagate(self.indptr, self.indices, self.scale, al[j], x, 1.0, out, self.k,
                           other)
            out, other = other, out
        return out

    def pair_grad(self, xbar: torch.Tensor, users, positives, negatives, *, loss_sum=None,
                  check_indices: bool = True, out: torch.Tensor | None = None):
        "(dloss/dxbar as a dense panel, the batch loss) of one batch of node numbers"
        lib = _native.require_gpu()
        dev = self.dev
        users, positives = _i32_dev(users, dev).reshape(-1), _i32_dev(positives, dev).reshape(-1)
        negatives = _i32_dev(negatives, dev).reshape(-1)
        B = users.numel()
        if positives.numel() != B or negatives.numel() != B or B < 1:
            raise ValueError("batch arrays disagree in length")
        if check_indices:
            for name, t in (("users", users), ("positives", positives), ("negatives", negatives)):
                if int(t.min()) < 0 or int(t.max()) >= self.n:
                    raise ValueError(f"{name} outside [0, {self.n})")
        if self._ws is None or self._ws_batch < B:
            self._ws = torch.empty(lib.lk_lgcn_pair_grad_workspace_bytes(B), dtype=torch.uint8,
                                   device=dev)
            self._ws_batch = B
        g = self._work[2] if out is None else out
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.lk_lgcn_pair_grad(_ptr(xbar), self.n, self.k, self.X.shape[1],
                                    _native.FLEXMF_LOSSES[self.loss], _ptr(users),
                                    _ptr(positives), _ptr(negatives), B, _ptr(self._ws), _ptr(g),
                                    _ptr(loss), _ptr(loss_sum), _stream()), "lk_lgcn_pair_grad")
        return g, loss

    def step(self, users, positives, negatives, *, loss_sum=None,
             check_indices: bool = True) -> torch.Tensor:
        "One training step; returns the batch loss (device, 1 element), nothing synchronised."
        xbar = self.propagate(self.X)
        g, loss = self.pair_grad(xbar, users, positives, negatives, loss_sum=loss_sum,
                                 check_indices=check_indices)
        grad = self.propagate(g)
        self.steps += 1
        adamw_dense(self.X, self.exp_avg, self.exp_avg_sq, grad, self.k, step=self.steps,
                    learning_rate=self.learning_rate, weight_decay=self.weight_decay)
        return loss

    def final_embeddings(self) -> np.ndarray:
        "The propagated, blended embeddings xbar [n x k] on the host: one forward pass."
        return self.propagate(self.X)[:, :self.k].cpu().numpy()

    def host_table(self) -> np.ndarray:
        "The embedding table X [n x k] on the host."
        return self.X[:, :self.k].cpu().numpy()

    def load_table(self, table) -> None:
        table = np.asarray(table, dtype=np.float32)
        if table.shape != (self.n, self.k):
            raise ValueError(f"the embedding table is {(self.n, self.k)}, got {table.shape}")
        self.X[:, :self.k] = torch.from_numpy(np.ascontiguousarray(table)).to(self.dev)


# ---- hierarchical Poisson factorization (csrc/hpf.hip) -------------------------------------------
def hpf_rates_block() -> int:
    "The rows behind one partial column sum of ``lk_hpf_rates`` (lk_hpf_rates_block)."
    return int(_native.load().lk_hpf_rates_block())


def _hpf_panels(k: int, *panels) -> tuple[int, int]:
    n, ld = panels[0].shape
    assert ld == padded_dim(k)
    for p in panels:
        assert p.dtype == torch.float32 and p.is_contiguous() and tuple(p.shape) == (n, ld)
    return n, ld


def hpf_expect_log(shp: torch.Tensor, rte: torch.Tensor, k: int,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    "``psi(shp) - log(rte)`` of two padded panels, float64 rounded once (lk_hpf_expect_log)."
    lib = _native.require_gpu()
    if out is None:
        out = torch.empty_like(shp)
    n, ld = _hpf_panels(k, shp, rte, out)
    check(lib.lk_hpf_expect_log(_ptr(shp), _ptr(rte), n, int(k), ld, _ptr(out), _stream()),
          "lk_hpf_expect_log")
    return out


def hpf_shape_pass(csr: DeviceCSR, e_rows: torch.Tensor, e_cols: torch.Tensor, k: int,
                   prior: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """
    ``out[r] = prior + sum_e y_e softmax(e_rows[r] + e_cols[col_e])`` over the entries of CSR row
    r (lk_hpf_shape_pass): the shape update of the rows' side, a padded panel [rows x LD].
    """
    lib = _native.require_gpu()
    n_rows, n_cols = csr.shape
    if out is None:
        out = torch.empty_like(e_rows)
    _, ld = _hpf_panels(k, e_rows, out)
    _hpf_panels(k, e_cols)
    assert e_rows.shape[0] == n_rows and e_cols.shape[0] == n_cols
    assert csr.values is not None and csr.values.dtype == torch.float32
    check(lib.lk_hpf_shape_pass(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                                _ptr(csr.values), n_rows, n_cols, csr.nnz, _ptr(e_rows),
                                _ptr(e_cols), int(k), ld, float(prior), _ptr(out), _stream()),
          "lk_hpf_shape_pass")
    return out


def hpf_rates(shp: torch.Tensor, k: int, shp_hyper: float, prior_ratio: float,
              hyper_rte: torch.Tensor, other_colsum: torch.Tensor, rte: torch.Tensor,
              mean: torch.Tensor, colsum: torch.Tensor, ws: torch.Tensor | None = None) -> None:
    """
    The rate update of one side (lk_hpf_rates): ``rte = shp_hyper / hyper_rte + other_colsum``,
    ``mean = shp / rte``, then ``hyper_rte = prior_ratio + mean.sum(1)`` (in place) and
    ``colsum = mean.sum(0)``, both float64 sums of fixed order rounded once.
    """
    lib = _native.require_gpu()
    n, ld = _hpf_panels(k, shp, rte, mean)
    for v, m in ((hyper_rte, n), (other_colsum, k), (colsum, k)):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == m
    need = lib.lk_hpf_rates_workspace_bytes(n, int(k))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=shp.device)
    assert ws.numel() * ws.element_size() >= need
    check(lib.lk_hpf_rates(_ptr(shp), n, int(k), ld, float(shp_hyper), float(prior_ratio),
                           _ptr(hyper_rte), _ptr(other_colsum), _ptr(rte), _ptr(mean),
                           _ptr(colsum), _ptr(ws), _stream()), "lk_hpf_rates")


def hpf_loglik_rows(csr: DeviceCSR, theta: torch.Tensor, beta: torch.Tensor,
                    k: int) -> torch.Tensor:
    "Per row ``sum_e y_e log(theta[r] . beta[col_e])`` in float64 (lk_hpf_loglik_rows)."
    lib = _native.require_gpu()
    n_rows, n_cols = csr.shape
    _, ld = _hpf_panels(k, theta)
    _hpf_panels(k, beta)
    assert theta.shape[0] == n_rows and beta.shape[0] == n_cols
    assert csr.values is not None and csr.values.dtype == torch.float32
    out = torch.empty(n_rows, dtype=torch.float64, device=theta.device)
    check(lib.lk_hpf_loglik_rows(_ptr(csr.indptr), 1 if csr.is64 else 0, _ptr(csr.indices),
                                 _ptr(csr.values), n_rows, n_cols, csr.nnz, _ptr(theta),
                                 _ptr(beta), int(k), ld, _ptr(out), _stream()),
          "lk_hpf_loglik_rows")
    return out


def _f64_rowsum_f32(x: np.ndarray, first: float) -> np.ndarray:
    "``first + sum_c x[:, c]`` in float64 in column order, rounded to float32 once"
    s = np.zeros(len(x), dtype=np.float64)
    for c in range(x.shape[1]):
        s += x[:, c]
    return (first + s).astype(np.float32)


class HPFState:
    """
    The variational state of a hierarchical Poisson factorization in HBM: the count matrix Y and
    its transpose (CSR), the shape, rate and mean panels of the users (gamma, theta) and of the
    items (lambda, beta) [n x LD], the hyper-rates kappa [users] and tau [items], the column sums
    T = sum_u theta and S = sum_i beta [k], two E panels and the rate pass's workspace.

    ``start``: the four host panels gamma_shp, gamma_rte, lambda_shp, lambda_rte ([n x k]
    float32); the means, hyper-rates and column sums of the start are formed on the host as
    ``lk_hpf_rates`` forms them.  ``iterate`` queues whole iterations -- two
    ``lk_hpf_expect_log``, two ``lk_hpf_shape_pass``, two ``lk_hpf_rates`` -- and synchronises
    nothing; ``loglik`` does.
    """

    def __init__(self, csr: DeviceCSR, start, *, a: float = 0.3, a_prime: float = 0.3,
                 b_prime: float = 1.0, c: float = 0.3, c_prime: float = 0.3,
                 d_prime: float = 1.0, lgamma_sum: float = 0.0):
        g_shp, g_rte, l_shp, l_rte = (np.ascontiguousarray(p, dtype=np.float32) for p in start)
        n_users, n_items = csr.shape
        self.k = k = g_shp.shape[1]
        if not 1 <= k <= _native.FLEXMF_MAX_K:
            raise ValueError(f"unsupported embedding size {k} "
                             f"(supported: 1..{_native.FLEXMF_MAX_K})")
        if g_shp.shape != (n_users, k) or g_rte.shape != (n_users, k) or \
                l_shp.shape != (n_items, k) or l_rte.shape != (n_items, k):
            raise ValueError("the start panels do not fit the matrix")
        for name, v in (("a", a), ("a_prime", a_prime), ("b_prime", b_prime), ("c", c),
                        ("c_prime", c_prime), ("d_prime", d_prime)):
            if not v > 0:
                raise ValueError(f"{name} must be positive, got {v}")
        self.dev = dev = csr.indices.device
        self.csr, self.csr_t = csr, csr_transpose(csr)
        self.a, self.c = float(a), float(c)
        self.k_shp, self.t_shp = a_prime + k * a, c_prime + k * c
        self.k_ratio, self.t_ratio = a_prime / b_prime, c_prime / d_prime
        self.lgamma_sum = float(lgamma_sum)
        theta, beta = g_shp / g_rte, l_shp / l_rte

        def vec(x):
            return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

        self.g_shp, self.g_rte = to_device_padded(g_shp, dev), to_device_padded(g_rte, dev)
        self.l_shp, self.l_rte = to_device_padded(l_shp, dev), to_device_padded(l_rte, dev)
        self.theta, self.beta = to_device_padded(theta, dev), to_device_padded(beta, dev)
        self.k_rte = vec(_f64_rowsum_f32(theta, self.k_ratio))
        self.t_rte = vec(_f64_rowsum_f32(beta, self.t_ratio))
        self.T = vec(theta.sum(axis=0, dtype=np.float64))
        self.S = vec(beta.sum(axis=0, dtype=np.float64))
        self.e_u, self.e_i = torch.empty_like(self.g_shp), torch.empty_like(self.l_shp)
        lib = _native.require_gpu()
        self._ws = torch.empty(max(lib.lk_hpf_rates_workspace_bytes(n_users, k),
                                   lib.lk_hpf_rates_workspace_bytes(n_items, k)),
                               dtype=torch.uint8, device=dev)
        self.iterations = 0

    def iterate(self, n: int = 1) -> None:
        "``n`` iterations, queued: users against the items as they stand, then items"
        k = self.k
        for _ in range(int(n)):
            hpf_expect_log(self.g_shp, self.g_rte, k, self.e_u)
            hpf_expect_log(self.l_shp, self.l_rte, k, self.e_i)
            hpf_shape_pass(self.csr, self.e_u, self.e_i, k, self.a, self.g_shp)
            hpf_shape_pass(self.csr_t, self.e_i, self.e_u, k, self.c, self.l_shp)
            hpf_rates(self.g_shp, k, self.k_shp, self.k_ratio, self.k_rte, self.S, self.g_rte,
                      self.theta, self.T, self._ws)
            hpf_rates(self.l_shp, k, self.t_shp, self.t_ratio, self.t_rte, self.T, self.l_rte,
                      self.beta, self.S, self._ws)
            self.iterations += 1

    def loglik(self) -> float:
        """``sum y log(theta . beta) - sum_c T_c S_c - sum lgamma(y + 1)``: the rows from
        ``lk_hpf_loglik_rows`` added on the host in row order (synchronises)."""
        rows = hpf_loglik_rows(self.csr, self.theta, self.beta, self.k).cpu().numpy()
        ts = torch.stack([self.T, self.S]).cpu().numpy().astype(np.float64)
        data = float(np.cumsum(rows)[-1]) if len(rows) else 0.0
        return data - float(np.cumsum(ts[0] * ts[1])[-1]) - self.lgamma_sum

    def host_factors(self) -> tuple[np.ndarray, np.ndarray]:
        "(theta [users x k], beta [items x k]) on the host"
        return to_host_unpadded(self.theta, self.k), to_host_unpadded(self.beta, self.k)


# ---- non-negative matrix factorization (csrc/nmf.hip) ----------------------------------------
def nmf_max_k() -> int:
    "The largest ``k`` ``lk_nmf_cd_sweep`` serves (lk_nmf_max_k)."
    return int(_native.load().lk_nmf_max_k())


def nmf_cd_sweep(w: torch.Tensor, hht: torch.Tensor, xht: torch.Tensor, l1_reg: float,
                 out: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
    """
    One coordinate sweep over the rows of the padded panel ``w`` [n x KP], in place
    (lk_nmf_cd_sweep: sklearn's ``_update_cdnmf_fast`` in float32, bit for bit): ``hht`` [k x k]
    is ``Ht^T Ht + l2_reg I`` and ``xht`` [n x KP] the padded ``X Ht``, from which ``l1_reg`` is
    subtracted.  Returns the sweep's violation ``sum |pg|`` as a device float64 [1] (``out``, if
    given); nothing is read back here.  ``ValueError`` for a ``k`` above :func:`nmf_max_k`.
    """
    lib = _native.require_gpu()
    k = int(hht.shape[0])
    if not 1 <= k <= nmf_max_k():
        raise ValueError(f"nmf_cd_sweep: k = {k} outside 1..lk_nmf_max_k() = {nmf_max_k()}")
    kp = padded_dim(k)
    n = int(w.shape[0])
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (n, kp)
    assert xht.dtype == torch.float32 and xht.is_contiguous() and tuple(xht.shape) == (n, kp)
    assert hht.dtype == torch.float32 and hht.shape[1] == k and hht.stride(1) == 1
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=w.device)
    assert out.dtype == torch.float64 and out.numel() == 1
    need = lib.lk_nmf_workspace_bytes(n)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=w.device)
    check(lib.lk_nmf_cd_sweep(_ptr(w), n, k, kp, _ptr(hht), hht.stride(0), _ptr(xht),
                              float(l1_reg), _ptr(out), _ptr(ws), _stream()), "lk_nmf_cd_sweep")
    return out


def nmf_fit(csr: DeviceCSR, csr_t: DeviceCSR, w0: np.ndarray, h0: np.ndarray, max_iter: int,
            tol: float, l1_w: float = 0.0, l1_h: float = 0.0, l2_w: float = 0.0,
            l2_h: float = 0.0, *, stats: dict | None = None):
    """
    Frobenius NMF by coordinate descent, sklearn's ``_fit_coordinate_descent`` in float32: from
    ``w0`` [n_rows x k] and ``h0`` [k x n_cols], every iteration updates W (``HHt = Ht^T Ht + l2_w
    I`` by lk_gramian, ``XHt = X Ht`` by lk_csr_spmm, then lk_nmf_cd_sweep with ``l1_w``) and then
    Ht the same way on ``csr_t`` (:func:`csr_transpose`, formed once) with W.  The violation of an
    iteration is the sum of its two sweeps'; the fit stops when the first iteration's is 0 or once
    ``violation / violation_init <= tol`` -- the two float64 values are the one read-back of an
    iteration.

    Returns (W f32 [n_rows x k], H f32 [k x n_cols], n_iter, the violations of the iterations run)
    on the host.  ``stats`` (a dict, for the timing tool): the stream is synchronised around every
    step and the dict receives the seconds spent in ``gramian``, ``spmm`` and ``sweep``.
    """
    from time import perf_counter

    n_rows, n_cols = csr.shape
    w0 = np.ascontiguousarray(w0, dtype=np.float32)
    ht0 = np.ascontiguousarray(np.asarray(h0, dtype=np.float32).T)
    k = w0.shape[1]
    if not 1 <= k <= nmf_max_k():
        raise ValueError(f"nmf_fit: k = {k} outside 1..lk_nmf_max_k() = {nmf_max_k()}")
    if w0.shape != (n_rows, k) or ht0.shape != (n_cols, k):
        raise ValueError(f"nmf_fit: the start {w0.shape} x {ht0.T.shape} does not fit the "
                         f"matrix {csr.shape}")
    if tuple(csr_t.shape) != (n_cols, n_rows) or csr_t.nnz != csr.nnz:
        raise ValueError("nmf_fit: csr_t is not the transpose of csr")
    dev = csr.indices.device
    w, ht = to_device_padded(w0, dev), to_device_padded(ht0, dev)
    gramian = Gramian(k, dev)
    hht = torch.empty((k, k), dtype=torch.float32, device=dev)
    viol = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(_native.load().lk_nmf_workspace_bytes(max(n_rows, n_cols)),
                     dtype=torch.uint8, device=dev)
    if stats is not None:
        stats.update(gramian=0.0, spmm=0.0, sweep=0.0)

    def step(key, fn, *a):
        if stats is None:
            return fn(*a)
        torch.cuda.synchronize(dev)
        t0 = perf_counter()
        out = fn(*a)
        torch.cuda.synchronize(dev)
        stats[key] += perf_counter() - t0
        return out

    def half(mat, this, other, l1, l2, out):
        step("gramian", gramian, other, l2, hht)
        xht = step("spmm", csr_spmm, mat, other, k)
        step("sweep", nmf_cd_sweep, this, hht, xht, l1, out, ws)

    history: list[float] = []
    n_iter = 0
    for n_iter in range(1, int(max_iter) + 1):
        half(csr, w, ht, l1_w, l2_w, viol[0:1])
        half(csr_t, ht, w, l1_h, l2_h, viol[1:2])
        v = viol.cpu().numpy()
        history.append(float(v[0] + v[1]))
        if history[0] == 0 or history[-1] / history[0] <= tol:
            break
    return (to_host_unpadded(w, k), np.ascontiguousarray(to_host_unpadded(ht, k).T), n_iter,
            np.asarray(history, dtype=np.float64))


# ---- FunkSVD (csrc/funksvd.hip) --------------------------------------------------------------
# sample-steps (samples x epochs) one launch may hold: the kernel walks 1.7e8 to 1.9e8 samples a
# second (profiles/funksvd_mi355x.json), so a launch ends within 0.4 s
FUNKSVD_STEP_BUDGET = 1 << 26


@dataclass
class FunkSVDPlan:
    """The level schedule of a shuffled sample list (lk_funksvd_plan_levels / _order), on the
    host: ``order`` int64 [n] (sample positions in level order, ascending inside a level),
    ``level_ptr`` int64 [depth + 1], ``run_end`` int32 [depth] (the narrow-run marks) and
    ``level`` int32 [n] (each sample's level).  ``from_recurrence``: :func:`funksvd_plan` made it
    (a schedule a caller assigned is checked for repeats before it is run)."""

    order: np.ndarray
    level_ptr: np.ndarray
    run_end: np.ndarray
    level: np.ndarray
    from_recurrence: bool = False

    @property
    def depth(self) -> int:
        return len(self.level_ptr) - 1


def funksvd_lds_column_bytes() -> int:
    "The bytes of feature columns ``lk_funksvd_train_feature`` keeps in LDS."
    return int(_native.load().lk_funksvd_lds_column_bytes())


def funksvd_plan(users: np.ndarray, items: np.ndarray, n_users: int, n_items: int) -> FunkSVDPlan:
    """
    The level schedule of the samples ``(users[s], items[s])`` in their (shuffled) order:
    ``level(s) = 1 + max(level of the previous sample of the user, ... of the item)``, one
    sequential pass and one stable counting sort in the native library, on the host (no device
    is needed).  ``ValueError`` for a number outside ``n_users`` / ``n_items``.
    """
    lib = _native.load()
    users = np.ascontiguousarray(users, dtype=np.int32)
    items = np.ascontiguousarray(items, dtype=np.int32)
    n = len(users)
    if users.shape != (n,) or items.shape != (n,):
        raise ValueError("funksvd_plan: users and items must be vectors of one length")
    level = np.empty(n, np.int32)
    depth = ctypes.c_int32(0)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib.lk_funksvd_plan_levels(hp(users), hp(items), n, int(n_users), int(n_items),
                                     hp(level), ctypes.byref(depth)), "lk_funksvd_plan_levels")
    plan = funksvd_plan_of_levels(level, depth.value)
    plan.from_recurrence = True
    return plan


def funksvd_plan_of_levels(level: np.ndarray, depth: int | None = None) -> FunkSVDPlan:
    """
    The plan of a given level assignment (lk_funksvd_plan_order: the stable counting sort and the
    narrow-run marks).  Any assignment in which no user and no item repeats inside a level and
    every user's and item's samples keep their order is a schedule with the sequential walk's
    bits; :func:`funksvd_plan` makes the shallowest one.
    """
    lib = _native.load()
    level = np.ascontiguousarray(level, dtype=np.int32)
    n = len(level)
    if depth is None:
        depth = int(level.max()) + 1 if n else 0
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    order = np.empty(n, np.int64)
    level_ptr = np.empty(depth + 1, np.int64)
    run_end = np.empty(depth, np.int32)
    check(lib.lk_funksvd_plan_order(hp(level), n, depth, hp(order), hp(level_ptr), hp(run_end)),
          "lk_funksvd_plan_order")
    return FunkSVDPlan(order, level_ptr, run_end, level)


def funksvd_fit(users: np.ndarray, items: np.ndarray, ratings: np.ndarray, est: np.ndarray,
                n_users: int, n_items: int, k: int, epochs: int, lr: float, reg: float,
                rmin: float = -np.inf, rmax: float = np.inf, *, initial: float = 0.1,
                plan: FunkSVDPlan | None = None, dev=None, global_columns: bool = False,
                step_budget: int | None = None, stats: dict | None = None):
    """
    The reference's FunkSVD training loop (funksvd.py:148-190) on the device, bit for bit: from
    the shuffled samples (``users``, ``items`` int32, ``ratings`` float32) and their initial
    estimates ``est`` (float32; not modified), ``k`` features one after the other, ``epochs``
    epochs each, by ``lk_funksvd_train_feature`` over the samples in level order
    (:func:`funksvd_plan`, made here unless ``plan`` is given).  The level-ordered arrays are
    uploaded once; feature f trains with ``trail = initial * initial * (k - f - 1)`` and leaves
    its clipped contribution in the estimates for the next.

    A feature's epochs are split over several launches so that none holds more than
    ``step_budget`` (default :data:`FUNKSVD_STEP_BUDGET`) sample-steps, which changes no bit.
    ``global_columns`` (a test hook) keeps the feature columns in global memory at any size.

    Returns (user embeddings f32 [n_users x k], item embeddings f32 [n_items x k], the epochs'
    training RMSE f64 [k x epochs]) on the host.  ``stats`` (a dict, for the timing tool)
    receives ``plan_seconds``, ``train_seconds`` (the launches, synchronised), ``depth``,
    ``epochs_per_launch`` and ``sse`` (the epochs' squared errors as the kernel summed them).
    """
    from time import perf_counter

    lib = _native.require_gpu()
    dev = device(dev)
    users = np.ascontiguousarray(users, dtype=np.int32)
    items = np.ascontiguousarray(items, dtype=np.int32)
    ratings = np.ascontiguousarray(ratings, dtype=np.float32)
    est = np.ascontiguousarray(est, dtype=np.float32)
    n = len(users)
    if not (users.shape == items.shape == ratings.shape == est.shape == (n,)):
        raise ValueError("funksvd_fit: users, items, ratings and est must be vectors of one length")
    k, epochs = int(k), int(epochs)
    if k < 1 or epochs < 1:
        raise ValueError(f"funksvd_fit: k = {k} and epochs = {epochs} must be positive")
    t0 = perf_counter()
    if plan is None:
        plan = funksvd_plan(users, items, n_users, n_items)
    elif not plan.from_recurrence:  # a caller's schedule: two samples of a level share nothing
        if len(plan.level) != n:
            raise ValueError("funksvd_fit: the plan does not belong to these samples")
        for ent, count in ((users, n_users), (items, n_items)):
            key = plan.level.astype(np.int64) * max(int(count), 1) + ent
            if len(np.unique(key)) != n:
                raise ValueError("funksvd_fit: a user or an item repeats inside a level")
    t_plan = perf_counter() - t0
    ptr = plan.level_ptr
    if len(plan.order) != n or len(plan.run_end) != plan.depth or ptr[0] != 0 or ptr[-1] != n \
            or (np.diff(ptr) < 0).any():
        raise ValueError("funksvd_fit: the plan does not belong to these samples")
    # the run marks address level_ptr and size the kernel's stage: held to lk_funksvd_plan_order's
    at = np.arange(plan.depth)
    run = plan.run_end > at
    if (plan.run_end < at).any() or (plan.run_end > plan.depth).any() or \
            (ptr[plan.run_end[run]] - ptr[at[run]] > lib.lk_funksvd_stage_samples()).any() or \
            (np.diff(ptr)[run] > lib.lk_funksvd_narrow_width()).any():
        raise ValueError("funksvd_fit: the plan's narrow-run marks are not lk_funksvd_plan_order's")
    if n and (users.min() < 0 or users.max() >= n_users or items.min() < 0
              or items.max() >= n_items):
        raise ValueError("funksvd_fit: a sample's user or item number is out of range")
    budget = FUNKSVD_STEP_BUDGET if step_budget is None else int(step_budget)
    per_launch = max(1, min(epochs, budget // max(n, 1)))

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_users, d_items = up(users[plan.order]), up(items[plan.order])
    d_ratings, d_est = up(ratings[plan.order]), up(est[plan.order])
    d_ptr, d_run = up(ptr), up(plan.run_end)
    # one feature's column is one contiguous row of these
    d_ut = torch.full((k, int(n_users)), float(initial), dtype=torch.float32, device=dev)
    d_it = torch.full((k, int(n_items)), float(initial), dtype=torch.float32, device=dev)
    d_sse = torch.zeros((k, epochs), dtype=torch.float64, device=dev)
    flags = _native.FUNKSVD_GLOBAL_COLUMNS if global_columns else 0
    torch.cuda.synchronize(dev)
    t0 = perf_counter()
    for f in range(k):
        trail = initial * initial * (k - f - 1)  # funksvd.py:174, in Python floats
        done = 0
        while done < epochs:
            e = min(per_launch, epochs - done)
            check(lib.lk_funksvd_train_feature(
                _ptr(d_users), _ptr(d_items), _ptr(d_ratings), _ptr(d_est), _ptr(d_ptr),
                _ptr(d_run), plan.depth, _ptr(d_ut[f]), _ptr(d_it[f]), int(n_users),
                int(n_items), e, int(done + e == epochs), float(lr), float(reg), float(trail),
                float(rmin), float(rmax), flags, _ptr(d_sse[f, done:]), _stream()),
                "lk_funksvd_train_feature")
            done += e
    torch.cuda.synchronize(dev)
    t_train = perf_counter() - t0
    sse = d_sse.cpu().numpy()
    if stats is not None:
        stats.update(plan_seconds=t_plan, train_seconds=t_train, depth=plan.depth,
                     epochs_per_launch=per_launch, sse=sse)
    rmse = np.sqrt(sse / max(n, 1))  # funksvd.rs:126
    return (np.ascontiguousarray(d_ut.cpu().numpy().T), np.ascontiguousarray(d_it.cpu().numpy().T),
            rmse)
