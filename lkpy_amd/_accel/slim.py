"""``lenskit._accel.slim`` stand-in (src/accel/slim/mod.rs:58-301)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _device as D
from ..parallel import AccelTask
from ._util import as_csr_arrays
from .knn import _sim_chunk


def _check_structure(name: str, offsets: np.ndarray, indices: np.ndarray, shape) -> None:
    """
    What the kernels rely on (``CSRStructure::from_arrow`` hands the reference a checked array):
    monotone offsets, every index inside the dimension, no row naming a column twice -- the lanes
    of a wave walk the entries of one row side by side.
    """
    n_rows, n_cols = shape
    if len(offsets) != n_rows + 1 or (len(offsets) and (offsets[0] != 0 or
                                                         np.any(np.diff(offsets) < 0))):
        raise ValueError(f"{name}: invalid row offsets")
    nnz = int(offsets[-1]) if len(offsets) else 0
    if len(indices) < nnz:
        raise ValueError(f"{name}: fewer indices than the offsets claim")
    idx = indices[:nnz]
    if nnz and (idx.min() < 0 or idx.max() >= n_cols):
        raise ValueError(f"{name}: column index out of range")
    if nnz:
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(offsets))
        cell = rows * max(n_cols, 1) + idx
        cell.sort()
        if np.any(cell[1:] == cell[:-1]):
            raise ValueError(f"{name}: a row names a column twice")


def train_slim(ui_matrix, iu_matrix, l1_reg: float, l2_reg: float, max_iters: int,
               max_nbrs: int | None) -> AccelTask:
    """
    Learn SLIM regression weights (mod.rs:58-93): ``ui_matrix`` users x items and ``iu_matrix``
    items x users, structure only (values, if any, are ignored), 32- or 64-bit offsets.  Returns
    a task yielding a LIST of ``pa.LargeListArray`` chunks -- the TRANSPOSED weight matrix, rows
    = target items in item order, sorted by column -- which the caller feeds to
    ``pa.chunked_array(...).combine_chunks()`` and ``SparseRowArray.from_array``
    (src/lenskit/knn/slim.py:115-116).  The shape errors are the reference's, raised here on the
    host before any device work.
    """
    uo, uidx, _uv, ushape = as_csr_arrays(ui_matrix)
    io, iidx, _iv, ishape = as_csr_arrays(iu_matrix)
    if ushape[0] != ishape[1]:
        raise ValueError("user count mismatch")  # mod.rs:71-73
    if ushape[1] != ishape[0]:
        raise ValueError("item count mismatch")  # mod.rs:74-76
    if int(uo[-1]) != int(io[-1]):
        raise ValueError("rating count mismatch")  # mod.rs:77-79
    n_users, n_items = ushape
    _check_structure("ui_matrix", uo, uidx, ushape)
    _check_structure("iu_matrix", io, iidx, ishape)
    if int(max_iters) < 1:
        raise ValueError("max_iters must be positive")

    def run(task: AccelTask):
        dev = D.device()
        dt = np.int64 if (uo.dtype == np.int64 or io.dtype == np.int64) else np.int32

        def upload(off, idx, shape):
            # (np.array: Arrow buffers are read-only views; torch wants writable host memory)
            h = np.array(off, dtype=dt)
            return D.DeviceCSR(torch.from_numpy(h).to(dev),
                               torch.from_numpy(np.array(idx[:int(off[-1])], np.int32)).to(dev),
                               None, shape, h)

        ui = upload(uo, uidx, ushape)
        iu = upload(io, iidx, ishape)
        ctl = D.TaskCtl()
        task.attach(ctl)  # cancel() / current_progress() reach the running trainer
        out = D.slim_train(ui, iu, l1_reg, l2_reg, max_iters, max_nbrs, ctl=ctl,
                           on_batch=task.set_progress)
        task.set_progress(n_items)
        return [_sim_chunk(out.indptr.cpu().numpy(), D.to_host(out.indices),
                           D.to_host(out.values), n_items)]

    return AccelTask(run, total=n_items)
