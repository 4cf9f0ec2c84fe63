"""
Stochastic top-N ranking: ``lenskit.stochastic.StochasticTopNRanker``
(src/lenskit/stochastic/_ranker.py:19-156) -- a ranking sampled from the Plackett-Luce
distribution over the (transformed) scores by exponential-sort sampling -- on the device, for one
list, for whole panels of score rows and for ragged batches of candidate lists
(:func:`rank_ragged`, ``lk_ragged_stochastic_keys``), with many samples per row.

The keys come from ``lk_stochastic_row_stats`` / ``lk_stochastic_keys`` (csrc/stochastic.hip), the
list from ``lk_argtopn`` + ``lk_take_scores``.  The key is ``g = log w~ - log(-log u)``; the
reference's ``log(u) / max(w, tiny)`` is ``-exp(-g)``, the same order.

**Random numbers.**  The reference draws from a NumPy generator derived per query
(``derivable_rng``, src/lenskit/random.py:269-345); a device kernel cannot reproduce that stream,
so the draws are defined here: Philox4x32-10 keyed by a 64-bit ``seed`` with the counter
``(item >> 2, sample, stream)``, one 64-bit *stream* per ranked row.

- ``seed``: ``np.random.SeedSequence(s).generate_state(1, np.uint64)[0]`` for the seed ``s`` of the
  ``rng`` spec (``None`` and a bare ``"user"``: fresh entropy; a ``Generator`` / ``BitGenerator``:
  one raw draw from it).
- ``rng="user"`` or ``(s, "user")``: the stream is the user id -- an integer id itself (mod 2^64),
  a ``str`` / ``bytes`` id folded the way the reference's ``_bytes_seed`` does (the four int32 words
  of its md5 digest XOR-ed, absolute value) -- so the same user always gets the same ranking, in
  any batch.  A query without a user id takes a counted stream, below.
- any other spec: the stream is ``(calls so far << 32) | row position`` -- every call (``__call__``,
  ``streams`` for a batch) draws afresh, the rows of one batch differ.

An item's draw is addressed by its *item number*: its number in the list's vocabulary (its
position for a list without one), the column of a panel.  One list and the same list inside a
batch therefore agree bit for bit.
"""

from __future__ import annotations

from typing import Any, Literal

import numpy as np
from pydantic import BaseModel

from ._streams import RowStreams, parse_rng, user_stream  # noqa: F401 (re-exported)
from .data import ItemList, RecQuery
from .pipeline import Component


def rank_panel(panel, streams, n: int, *, transform, scale: float, seed: int, excl=None,
               samples: int = 1, first_sample: int = 0, device_output: bool = False):
    """
    ``samples`` sampled rankings of every row of ``panel`` (device f32 [B x items]; non-finite
    and ``excl``-uded entries take no part) under the given transform, scale and seed: (item
    numbers int32 [B x S x n] with -1 padding, keys f32 [B x S x n] with NaN padding), sample
    ``first_sample + s`` at ``[:, s]``; ``n < 0``: every item.  The row statistics are computed
    once and one key panel is reused by every sample.
    """
    import torch

    from . import _device as D

    B, I = panel.shape
    cols = I if n < 0 else min(n, I)
    samples = int(samples)
    idx = torch.full((B, samples, max(n, cols)), -1, dtype=torch.int32, device=panel.device)
    keys = torch.full(idx.shape, float("nan"), dtype=torch.float32, device=panel.device)
    if B and cols and samples:
        d_streams = D._row_streams(streams, B, panel.device)
        buf = stats = None
        for s in range(samples):
            buf, stats = D.stochastic_keys(
                panel, d_streams, transform=transform, scale=scale, seed=seed,
                sample=first_sample + s, excl=excl, stats=stats, out=buf)
            picked = D.argtopn(buf, n)
            idx[:, s, :cols] = picked
            keys[:, s, :cols] = D.take_scores(buf, picked)
    if device_output:
        return idx, keys
    return D.to_host(idx), D.to_host(keys)


def rank_ragged(ptr, addr, payload, scores, widths, streams, n: int, *, transform, scale: float,
                seed: int, samples: int = 1, first_sample: int = 0, device_output: bool = False):
    """
    :func:`rank_panel` for ragged candidate lists, without a panel: list b is the entries
    ``ptr[b]:ptr[b + 1]`` (host int64 offsets from 0), entry t has the score ``scores[t]`` (device
    f32 [total], or a host array), the item number ``addr[t]`` that addresses its draw (host int32:
    strictly ascending inside a list and below ``widths[b]``, the length of the row the list would
    occupy in a panel) and the number ``payload[t]`` that the result carries for it (int32, host or
    device; None: the address; a negative one is dropped).  The keys are those of ``rank_panel``
    on the [1 x widths[b]] row holding the scores at the addresses (``lk_ragged_stochastic_keys``,
    computed once for every sample), the lists ``lk_ragged_topn`` of them: ties go to the lower
    position, which is the lower column.  Returns (payload int32 [B x S x n] padded with -1, keys
    f32 [B x S x n] padded with NaN), sample ``first_sample + s`` at ``[:, s]``; ``n < 0``: every
    entry, the width of the longest list.
    """
    import torch

    from . import _device as D

    samples, n = int(samples), int(n)
    keys, _stats, d_ptr, d_addr = D.ragged_stochastic_keys(
        ptr, addr, scores, widths, streams, transform=transform, scale=scale, seed=seed,
        samples=samples, first_sample=first_sample)
    h_ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
    B = len(h_ptr) - 1
    dev = keys.device
    if payload is None:
        d_payload = d_addr
    elif isinstance(payload, torch.Tensor):
        d_payload = payload
    else:
        d_payload = torch.from_numpy(np.ascontiguousarray(payload, dtype=np.int32)).to(dev)
    width = (int(np.diff(h_ptr).max()) if B else 0) if n < 0 else n
    idx = torch.full((B, samples, width), -1, dtype=torch.int32, device=dev)
    out = torch.full((B, samples, width), float("nan"), dtype=torch.float32, device=dev)
    if B and width and keys.shape[1]:
        for s in range(samples):
            i, k = D.ragged_topn(d_ptr, d_payload, keys[s], n, h_ptr)
            idx[:, s, :i.shape[1]] = i
            out[:, s, :i.shape[1]] = k
    if device_output:
        return idx, out
    return D.to_host(idx), D.to_host(out)


class StochasticTopNConfig(BaseModel, arbitrary_types_allowed=True):
    "src/lenskit/stochastic/_ranker.py:19-56"

    n: int | None = None  # the list length; -1 or None: every scored item
    rng: Any = None  # DerivableSeed: a seed, "user", or (seed, "user")
    transform: Literal["softmax", "linear"] | None = "softmax"
    scale: float = 1.0  # multiplies the scores before the transform (the softmax's beta)


class StochasticTopNRanker(RowStreams, Component):
    """
    Stochastic top-N ranking with an optional weight transformation (``StochasticTopNRanker``,
    _ranker.py:59-156).  ``__call__`` ranks one scored list; :meth:`rank_panel` ranks every row of
    a device panel of scores, ``samples`` times, from one statistics pass.
    """

    config: StochasticTopNConfig

    def __init__(self, config=None, **kwargs):
        if isinstance(config, dict) and isinstance(config.get("rng"), list):
            config = {**config, "rng": tuple(config["rng"])}  # (a TOML / JSON [seed, "user"])
        super().__init__(config, **kwargs)
        self._init_streams(self.config.rng)

    def _length(self, n: int | None) -> int:
        if n is None or n < 0:
            n = self.config.n or -1  # (_ranker.py:110-111)
        return int(n)

    # -- panels -------------------------------------------------------------------------------
    def rank_panel(self, panel, streams, n: int | None, *, excl=None, samples: int = 1,
                   first_sample: int = 0, device_output: bool = False):
        """
        ``samples`` sampled rankings of every row of ``panel`` (device f32 [B x items]; non-finite
        and ``excl``-uded entries take no part): (item numbers int32 [B x S x n] with -1 padding,
        keys f32 [B x S x n] with NaN padding), sample ``first_sample + s`` at ``[:, s]``.  The row
        statistics are computed once and one key panel is reused by every sample.
        """
        return rank_panel(panel, streams, self._length(n), transform=self.config.transform,
                          scale=self.config.scale, seed=self.seed, excl=excl, samples=samples,
                          first_sample=first_sample, device_output=device_output)

    def rank_ragged(self, ptr, addr, payload, scores, widths, streams, n: int | None, *,
                    samples: int = 1, first_sample: int = 0, device_output: bool = False):
        """
        ``samples`` sampled rankings of every list of a ragged batch of scored candidates
        (:func:`rank_ragged`) under the config's transform, scale and seed: the lists
        :meth:`sample` draws one by one, without their [1 x items] rows.
        """
        return rank_ragged(ptr, addr, payload, scores, widths, streams, self._length(n),
                           transform=self.config.transform, scale=self.config.scale,
                           seed=self.seed, samples=samples, first_sample=first_sample,
                           device_output=device_output)

    # -- one list -------------------------------------------------------------------------------
    def sample(self, items: ItemList, query=None, n: int | None = None, *, samples: int = 1,
               include_weights: bool = False) -> list[ItemList]:
        "``samples`` rankings of one scored list (``__call__`` is the first)."
        import torch

        from . import _device as D

        query = RecQuery.create(query)
        scores = items.scores()
        if scores is None:
            raise ValueError("item list must have scores")  # (_ranker.py:100-102)
        stream = self.streams(None if query.user_id is None else [query.user_id], 1)
        valid = np.isfinite(scores)
        if not valid.any():
            return [ItemList(items[valid], ordered=True) for _ in range(samples)]
        # a one-row panel over the item numbers: the kernels, and the draws, of a batch row
        if items.vocabulary is not None:
            nums, width = items.numbers(), len(items.vocabulary)
        else:
            nums, width = np.arange(len(items)), len(items)
        row = np.full((1, width), np.nan, dtype=np.float32)
        row[0, nums] = scores
        position = np.full(width, -1, dtype=np.int64)
        position[nums] = np.arange(len(items))
        idx, keys = self.rank_panel(torch.from_numpy(row).to(D.device()), stream, n,
                                    samples=samples)
        out = []
        for s in range(samples):
            keep = idx[0, s] >= 0
            g = keys[0, s][keep]
            ranked = items._take(position[idx[0, s][keep]], ordered=True)
            extra = {"weight": -np.exp(-g.astype(np.float64))} if include_weights else {}
            out.append(ItemList(ranked, ordered=True, scores=g, **extra))
        return out

    def __call__(self, items: ItemList, query=None, n: int | None = None, *,
                 include_weights: bool = False) -> ItemList:
        return self.sample(items, query, n, include_weights=include_weights)[0]
