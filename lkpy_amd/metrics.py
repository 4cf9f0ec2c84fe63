"""
Run evaluation: ``lenskit.metrics`` (src/lenskit/metrics/) with the per-list loop of
``MeasurementCollector.add_collection_measurements`` (``_collect.py:156-186``) replaced by ONE pass
over the whole batch on the device.

``lk_rank_stats`` (csrc/metrics.hip) yields, per list, the sufficient statistics of every built-in
ranking metric -- kept length, hit counts, first hit, the average-precision sum and the
rank-weighted hit sums per cutoff and weight table; ``lk_ideal_gain`` graded NDCG's denominator;
``lk_predict_errors`` the squared / absolute errors of RMSE / MAE.  The metric VALUES are composed
here, on the host, vectorised over the batch, with the reference's own expressions and corner
cases.  The rank-weight tables are computed on the host with the reference's NumPy expressions
(``ranking/_weighting.py:79-122``) and uploaded, so the kernels contain no ``log`` / ``exp`` and
any :class:`RankWeight` subclass works.

The exposure, diversity and popularity metrics (csrc/diversity.hip) need no test data:
``lk_item_exposure`` keeps the per-item totals of :class:`ListGini` / :class:`ExposureGini` on the
device across the collector's ``add_*`` calls, ``lk_list_category_stats`` yields the category
column-sum statistics of :class:`ILS` / :class:`Entropy` / :class:`RankBiasedEntropy` and
``lk_list_gather_mean`` the sums of :class:`MeanPopRank`.  The comparisons of two rankings
(rank-biased overlap, least item promoted) are in :mod:`lkpy_amd.reranking_metrics`.

There is no host-only implementation: ``measure_list`` on one pair of lists is the same path with
a batch of one.  Only :class:`FunctionMetric` (plain callables) runs list by list on the host.

Out of scope: ``weight_field=`` of RBP.
"""

from __future__ import annotations

import logging
import warnings
import weakref
from math import sqrt
from typing import Any, NamedTuple

import numpy as np
import pandas as pd

from .data import Dataset, ItemList, ItemListCollection, Vocabulary, _LazyLists, _RaggedLists
from .knn import DataWarning

_log = logging.getLogger(__name__)

UNKNOWN_ITEM = np.int32(0x7FFFFFFF)  # a ranked item no truth row can hold (keeps its rank)


# ---------------------------------------------------------------------------------------
# rank weights (ranking/_weighting.py:21-122)
# ---------------------------------------------------------------------------------------


class RankWeight:
    "Multiplicative rank weights; ranks start at 1 (``_weighting.py:21-54``)."

    def weight(self, ranks) -> np.ndarray:
        raise NotImplementedError()

    def log_weight(self, ranks) -> np.ndarray:
        return np.log(self.weight(ranks))

    def series_sum(self) -> float | None:
        return None

    def _table_key(self):
        return ("id", id(self))


class GeometricRankWeight(RankWeight):
    "``patience ** (rank - 1)`` (``_weighting.py:57-87``), the RBP model."

    def __init__(self, patience: float = 0.85):
        if not (0.0 < patience < 1.0):
            raise ValueError("patience must be in (0, 1)")
        self.patience = float(patience)

    def weight(self, ranks):
        return np.exp(self.log_weight(ranks))

    def log_weight(self, ranks):
        return np.log(self.patience) * (np.asarray(ranks) - 1)

    def series_sum(self) -> float:
        return 1 / (1 - self.patience)

    def _table_key(self):
        return ("geometric", self.patience)


class LogRankWeight(RankWeight):
    "``log(base) / log(max(rank, 2))`` or ``/ log(rank + offset)`` (``_weighting.py:89-122``)."

    def __init__(self, *, base: float = 2, offset: int = 0):
        if not base > 0:
            raise ValueError("base must be positive")
        if offset < 0:
            raise ValueError("offset must be non-negative")
        self.base = base
        self.offset = int(offset)

    def weight(self, ranks):
        ranks = np.asarray(ranks)
        if self.offset > 0:
            return np.log(self.base) / np.log(ranks + self.offset)
        else:
            return np.log(self.base) / np.log(np.maximum(ranks, 2))

    def _table_key(self):
        return ("log", self.base, self.offset)


_DEFAULT_LOG = LogRankWeight()

# ---------------------------------------------------------------------------------------
# metric classes: what each needs from the kernels (``_request``) and the reference's
# expression over the batch (``_compose``)
# ---------------------------------------------------------------------------------------


class Metric:
    "``lenskit.metrics.Metric`` (``_base.py:37-114``)."

    default: float | None = None
    _kind = "rank"

    @property
    def label(self) -> str:
        return self.__class__.__name__

    def __str__(self):
        return f"Metric {self.label}"

    def measure_list(self, output: ItemList, test: ItemList, /):
        "One pair of lists: the batched path with a batch of one."
        return _scalar(_measure_pairs([self], [output], [test])[0][0][0])

    def extract_list_metrics(self, data, /):
        return None

    def _summarize(self, values: np.ndarray, extra) -> dict:
        return _value_stats(values)


class ListMetric(Metric):
    "A metric with one value per list (``_base.py:117-146``)."

    default: float | None = 0.0

    def extract_list_metrics(self, data, /):
        return data


class FunctionMetric(ListMetric):
    "A plain ``f(output, test) -> float``: runs list by list on the host (``_base.py:149-162``)."

    _kind = "function"

    def __init__(self, function):
        self._function = function

    @property
    def label(self) -> str:
        return self._function.__name__

    def measure_list(self, output: ItemList, test: ItemList, /) -> float:
        return self._function(output, test)


class RankingMetricBase(Metric):
    "The ``n`` cutoff of the ranking metrics (``ranking/_base.py:16-73``)."

    n: int | None = None

    def __init__(self, n: int | None = None, *, k: int | None = None):
        if n is None and k is not None:
            warnings.warn("k= is deprecated, use n=", DeprecationWarning)
            n = k
        if n is not None and n < 0:
            raise ValueError("n must be positive or None")
        self.n = n

    @property
    def k(self):
        return self.n

    @property
    def label(self):
        name = self.__class__.__name__
        return f"{name}@{self.n}" if self.n is not None else name

    def _request(self, plan: "_RankPlan"):
        plan.need(self.n)

    def _compose(self, s: "_RankStats") -> np.ndarray:
        raise NotImplementedError()


def _nan_where(cond, values):
    out = np.asarray(values, dtype=np.float64).copy()
    out[cond] = np.nan
    return out


class Hit(ListMetric, RankingMetricBase):
    "``_hit.py:36-42``: NaN without test items, else 1 when any recommended item is one."

    def _compose(self, s):
        return _nan_where(s.n_test == 0, s.n_hits(self.n) > 0)


class RecipRank(ListMetric, RankingMetricBase):
    "``_recip.py:40-50``."

    def _compose(self, s):
        first = s.first_hit(self.n)
        val = np.zeros(s.B)
        np.divide(1.0, first, out=val, where=first > 0)  # 1.0 / (npz[0] + 1.0)
        return _nan_where(s.n_test == 0, val)


class Precision(ListMetric, RankingMetricBase):
    "``_pr.py:38-45``: NaN only for an empty list."

    def _compose(self, s):
        nrecs = s.n_recs(self.n)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _nan_where(nrecs == 0, s.n_hits(self.n) / nrecs)


class Recall(ListMetric, RankingMetricBase):
    "``_pr.py:64-71``: the denominator is ``min(len(test), n)``; 0 / 0 is NaN."

    def _compose(self, s):
        nrel = s.n_test if self.n is None else np.minimum(s.n_test, self.n)
        with np.errstate(divide="ignore", invalid="ignore"):
            return s.n_hits(self.n) / nrel


class AveragePrecision(ListMetric, RankingMetricBase):
    """
    ``_map.py:30-44``.  One deviation: with an empty test list and a non-empty recommendation
    list the reference divides by ``min(len(test), len(recs)) == 0`` in Python floats and raises
    ``ZeroDivisionError``; here that list's value is NaN.
    """

    def _compose(self, s):
        nrecs = s.n_recs(self.n)
        denom = np.minimum(s.n_test, nrecs)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _nan_where((nrecs == 0) | (denom == 0), s.ap_sum(self.n) / denom)


class DCG(ListMetric, RankingMetricBase):
    "``_dcg.py:148-221``."

    _warns_empty = True

    def __init__(self, n: int | None = None, *, k: int | None = None,
                 weight: RankWeight = _DEFAULT_LOG, gain: str | None = None):
        super().__init__(n, k=k)
        self.weight = weight
        self.gain = gain

    def _request(self, plan):
        plan.need(self.n, self.weight, self.gain or None)

    def _realized(self, s):
        if self.gain:
            val = s.g_hits(self.n, self.weight, self.gain)
            return _nan_where(s.gain_count(self.gain) == 0, val)  # _dcg.py:233-234
        return s.w_hits(self.n, self.weight)

    def _compose(self, s):
        return _nan_where(s.n_test == 0, self._realized(s))


class NDCG(DCG):
    "``_dcg.py:34-145``."

    def _request(self, plan):
        plan.need(self.n, self.weight, self.gain or None, ideal=bool(self.gain))

    def _compose(self, s):
        realized = self._realized(s)
        if self.gain:
            ideal = s.ideal(self.n, self.weight, self.gain)
            with np.errstate(divide="ignore", invalid="ignore"):
                val = realized / ideal
            val[ideal == 0] = 0.0  # _dcg.py:135-136
            val = _nan_where(s.gain_count(self.gain) == 0, val)
        else:
            n = s.n_test if not self.n else np.minimum(s.n_test, self.n)  # _dcg.py:140-143
            ideal = s.prefix(self.weight, n)  # fixed_dcg(n): np.sum over the prefix
            with np.errstate(divide="ignore", invalid="ignore"):
                val = realized / ideal
        return _nan_where(s.n_test == 0, val)


class RBP(ListMetric, RankingMetricBase):
    """``_rbp.py:40-162`` (without ``weight_field``).  A normalisation of 0 (an empty list with a
    weight that has no series sum, or ``normalize=True``) gives NaN where the reference's Python
    float division raises ``ZeroDivisionError``."""

    def __init__(self, n: int | None = None, *, k: int | None = None,
                 weight: RankWeight | None = None, patience: float = 0.85,
                 normalize: bool = False):
        super().__init__(n, k=k)
        self.patience = patience
        self.weight = GeometricRankWeight(patience) if weight is None else weight
        self.normalize = normalize

    def _request(self, plan):
        plan.need(self.n, self.weight)

    def _compose(self, s):
        k = s.n_recs(self.n)
        wmax = self.weight.series_sum()
        if self.normalize:
            norm = s.prefix(self.weight, np.minimum(s.n_test, k))
        elif wmax is not None:
            norm = wmax
        else:
            norm = s.prefix(self.weight, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _nan_where(s.n_test == 0, s.w_hits(self.n, self.weight) / norm)


# ---------------------------------------------------------------------------------------
# exposure, diversity and popularity (csrc/diversity.hip): metrics of the lists alone.  A metric
# launches its kernel over the batch's device lists numbered by ITS vocabulary (``_launch``) and
# composes the values from what the kernel left once everything is queued (``_finish``).
# ---------------------------------------------------------------------------------------


_SHARED: dict = {}  # (id(host object), tag) -> (weak reference to it, what was derived from it)


def _derived(source, tag, build):
    """
    What ``build()`` makes of the host object ``source`` (a normalised matrix, a device copy), made
    once per (object, tag) and kept while the object lives -- the rule of the components' device
    cache (the same object: the same state), held here per host object so that metric objects
    built from one matrix share one normalised form and one upload.  Nothing of it is pickled.
    """
    key = (id(source), tag)
    hit = _SHARED.get(key)
    if hit is None or hit[0]() is not source:
        _SHARED.pop(key, None)  # (a stale entry's device memory goes before the build)
        hit = _SHARED[key] = (weakref.ref(source, lambda _r, key=key: _SHARED.pop(key, None)),
                              build())
    return hit[1]


class _ListsMetric(RankingMetricBase):
    _kind = "lists"

    def measure_list(self, output: ItemList, test: ItemList | None = None, /):
        return _scalar(_measure_pairs([self], [output], [None])[0][0][0])

    @property
    def _cutoff(self) -> int:
        return 0 if self.n is None else int(self.n)


class GiniBase(_ListsMetric):
    """
    ``ranking/_gini.py:24-51``: no value per list; the per-item totals of a whole run
    (``GiniAccumulator``) stay on the device with the collector, and the summary is the Gini
    coefficient of their distribution.  Items the vocabulary does not know are skipped.
    """

    default = None
    weight: RankWeight | None = None

    def __init__(self, n: int | None = None, *, k: int | None = None,
                 items: "Vocabulary | Dataset"):
        super().__init__(n, k=k)
        self.item_vocab = items.items if isinstance(items, Dataset) else items

    def _numbers(self, output: ItemList) -> np.ndarray:
        recs = output if self.n is None else output[:self.n]
        return recs.numbers(vocabulary=self.item_vocab)

    def _launch(self, p: "_ListPass"):
        from . import _device as D

        totals = p.state.get(id(self))
        if totals is None:
            totals = p.state[id(self)] = p.zeros(len(self.item_vocab))
        lists = p.lists(self.item_vocab)
        if self.n != 0 and lists.shape[1] and len(self.item_vocab):
            D.item_exposure(lists, totals, self._cutoff,
                            None if self.weight is None else p.table(self.weight))
        return None

    def _finish(self, pending, B):
        return None

    def _summarize_state(self, totals) -> float:
        "``GiniAccumulator.accumulate`` (``_gini.py:131-133``)"
        from .stats import gini

        totals = np.zeros(len(self.item_vocab)) if totals is None else totals.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = totals / totals.sum()
        return gini(dist)


class ListGini(GiniBase):
    "``_gini.py:54-75``: the Gini coefficient of the number of lists each item appears in."

    def measure_list(self, output: ItemList, test=None, /):
        return (self._numbers(output), 1.0)


class ExposureGini(GiniBase):
    "``_gini.py:78-116``: the Gini coefficient of the items' total rank-weighted exposure."

    def __init__(self, n: int | None = None, *, k: int | None = None,
                 items: "Vocabulary | Dataset", weight: RankWeight = GeometricRankWeight()):
        super().__init__(n=n, k=k, items=items)
        self.weight = weight

    def measure_list(self, output: ItemList, test=None, /):
        ids = self._numbers(output)
        return (ids, self.weight.weight(np.arange(1, len(ids) + 1, dtype=np.int32)))


def normalize_rows(matrix, normalize: str | None):
    """
    ``normalize_matrix`` (data/matrix.py:643-678) on a dense array or any SciPy sparse matrix:
    ``"unit"`` divides every row by its L2 norm, ``"distribution"`` by its sum (a row of zeros
    stays).  Returns a float64 dense array or ``csr_array``.
    """
    import scipy.sparse as sps

    sparse = sps.issparse(matrix)
    matrix = sps.csr_array(matrix, dtype=np.float64) if sparse else \
        np.asarray(matrix, dtype=np.float64)
    if matrix.ndim != 2:
        raise ValueError("the category matrix must be two-dimensional")
    if normalize is None:
        return matrix
    if normalize == "unit":
        stats = sps.linalg.norm(matrix, axis=1) if sparse else np.linalg.norm(matrix, axis=1)
    elif normalize == "distribution":
        data = matrix.data if sparse else matrix
        if data.size and data.min() < 0:
            raise ValueError("Cannot normalize to distribution: negative values present")
        stats = np.asarray(matrix.sum(axis=1), dtype=np.float64)
    else:
        raise ValueError(f"invalid normalization {normalize}")
    stats = np.array(stats, dtype=np.float64).reshape(-1)
    stats[stats == 0] = 1.0
    if sparse:
        return sps.csr_array(matrix / stats[:, None])
    return matrix / stats[:, None]


class _CategoryMetric(ListMetric, _ListsMetric):
    """
    The metrics of an item x category matrix.  ``(dataset, attribute, n)`` as the reference
    (the matrix is ``dataset.item_attrs[attribute]``, its rows the dataset's items), or
    ``categories=`` (a dense array or any SciPy sparse matrix) with ``items=`` (the vocabulary of
    its rows).  The rows are normalised here as ``cat_matrix(normalize=...)`` does; metrics
    built from the same matrix object share the normalised matrix and its one copy in HBM.
    """

    _normalize: str | None = None
    _name = ""
    weight: RankWeight | None = None

    def __init__(self, dataset: Dataset | None = None, attribute: str | None = None,
                 n: int | None = None, *, categories=None, items: Vocabulary | None = None):
        super().__init__(n)
        from . import _device as D

        if dataset is not None:
            if categories is not None or items is not None:
                raise TypeError("give a dataset and attribute, or categories= and items=")
            if attribute is None:
                raise TypeError("a dataset needs the attribute's name")
            attrs = getattr(dataset, "item_attrs", {})
            if attribute not in attrs:
                raise KeyError(f"items have no attribute {attribute}")
            categories, items = attrs[attribute], dataset.items
        elif categories is None or items is None:
            raise TypeError("give a dataset and attribute, or categories= and items=")
        self.attribute = "categories" if attribute is None else attribute
        if not hasattr(categories, "tocsr"):
            categories = np.asarray(categories)  # (an array is itself: one matrix, one upload)
        mat = _derived(categories, ("rows", self._normalize),
                       lambda: normalize_rows(categories, self._normalize))
        if mat.shape[0] != len(items):
            raise ValueError(f"{mat.shape[0]} matrix rows for {len(items)} items")
        if mat.shape[1] > D.CATEGORY_MAX:
            raise ValueError(f"{mat.shape[1]} category columns: the device keeps a list's column "
                             f"sums in LDS and supports at most {D.CATEGORY_MAX}")
        self._cat_matrix = mat
        self._item_vocab = items

    @property
    def label(self):
        base = f"{self._name}({self.attribute})"
        return f"{base}@{self.n}" if self.n is not None else base

    def _device_matrix(self, dev):
        """the matrix as a CSR in HBM (a dense one keeps every column), uploaded once per
        normalised matrix -- which the metrics built from one source matrix share"""
        def upload():
            import scipy.sparse as sps

            from . import _device as D

            m = self._cat_matrix
            if sps.issparse(m):
                return D.DeviceCategories.from_scipy(m, dev)
            R, C = m.shape
            return D.DeviceCategories(_to_dev(np.arange(R + 1, dtype=np.int64) * C, dev),
                                      _to_dev(np.tile(np.arange(C, dtype=np.int32), R), dev),
                                      _to_dev(m.reshape(-1), dev), (R, C))

        return _derived(self._cat_matrix, ("device", str(dev)), upload)

    def _launch(self, p: "_ListPass"):
        from . import _device as D

        lists = p.lists(self._item_vocab)
        if self.n == 0 or self._cat_matrix.shape[1] == 0:
            return None
        return D.list_category_stats(lists, self._device_matrix(p.dev), self._cutoff,
                                     None if self.weight is None else p.table(self.weight))

    def _finish(self, pending, B):
        if pending is None:
            return np.full(B, np.nan)
        known, stats = pending
        return self._value(known.cpu().numpy().astype(np.int64), stats.cpu().numpy())


def _to_dev(arr, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


class ILS(_CategoryMetric):
    """
    ``ranking/_ils.py:18-104``: the mean pairwise cosine similarity of the known items' unit
    vectors, from the identity ``sum_{i<j} v_i . v_j = (|sum_i v_i|^2 - sum_i |v_i|^2) / 2``.
    NaN without a known item, 1.0 with one.
    """

    _normalize = "unit"
    _name = "ILS"

    def _value(self, k, stats):
        with np.errstate(divide="ignore", invalid="ignore"):
            val = ((stats[0] - stats[1]) / 2) / (k * (k - 1) / 2)
        val[k == 1] = 1.0
        return _nan_where(k == 0, val)


class Entropy(_CategoryMetric):
    "``ranking/_entropy.py:91-145``: Shannon entropy of the known items' category distribution."

    _normalize = "distribution"
    _name = "Entropy"

    def _value(self, k, stats):
        return _nan_where(k == 0, stats[2])


class RankBiasedEntropy(Entropy):
    """
    ``ranking/_entropy.py:148-206``.  One deviation: with an item the vocabulary does not know in
    the list, the reference multiplies the known items' rows by the weights of ALL ranks and
    fails on the shape mismatch; here every known item keeps the weight of its own rank.
    """

    _name = "RBEntropy"

    def __init__(self, dataset: Dataset | None = None, attribute: str | None = None,
                 n: int | None = None, *, weight: RankWeight | None = None, categories=None,
                 items: Vocabulary | None = None):
        super().__init__(dataset, attribute, n, categories=categories, items=items)
        self.weight = weight if weight is not None else GeometricRankWeight(0.85)


def popularity_quantiles(data: Dataset, count: str = "users") -> np.ndarray:
    """
    ``MeanPopRank.__init__`` (``ranking/_pop.py:59-73``): per item number the average rank of its
    count among the positive counts, divided by their number; 0 for an item without any.
    """
    if count == "users":  # distinct users: a repeated (user, item) pair counts once
        pairs = np.unique(data._rows.astype(np.int64) * max(data.item_count, 1) + data._cols)
        counts = np.bincount(pairs % max(data.item_count, 1), minlength=data.item_count)
    elif count == "interactions":
        w = data._attrs.get("count")
        counts = np.bincount(data._cols, weights=w, minlength=data.item_count)
    else:
        raise ValueError(f"invalid count {count}")
    table = np.zeros(data.item_count, dtype=np.float64)
    pos = np.flatnonzero(counts > 0)
    if len(pos):
        ranks = pd.Series(counts[pos]).rank(method="average", ascending=True)
        ranks /= len(pos)
        table[pos] = ranks.to_numpy()
    return table


class MeanPopRank(ListMetric, _ListsMetric):
    "``ranking/_pop.py:19-84``: the mean popularity quantile of the recommended items."

    def __init__(self, data: Dataset, *, n: int | None = None, k: int | None = None,
                 count: str = "users"):
        super().__init__(n, k=k)
        self._item_vocab = data.items
        self.item_ranks = popularity_quantiles(data, count)

    def _launch(self, p: "_ListPass"):
        from . import _device as D

        table = _derived(self.item_ranks, ("device", str(p.dev)),
                         lambda: _to_dev(self.item_ranks, p.dev))
        lists = p.lists(self._item_vocab)
        if self.n == 0:
            return None
        return D.list_gather_mean(lists, table, self._cutoff)

    def _finish(self, pending, B):
        if pending is None:
            return np.full(B, np.nan)
        sums, lens = (t.cpu().numpy() for t in pending)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _nan_where(lens == 0, sums / lens)


class PredictMetric(Metric):
    """``predict.py:37-111``: the two ``missing_*`` dispositions.  A prediction list holds every
    item once (the kernel matches a repeated item to its truth entry once per occurrence)."""

    default = None
    _kind = "predict"
    _root = False

    def __init__(self, missing_scores: str = "error", missing_truth: str = "error"):
        self.missing_scores = missing_scores
        self.missing_truth = missing_truth

    def measure_list(self, predictions: ItemList, test: ItemList | None = None, /):
        "-> (sum of squared / absolute errors, number of finite errors), ``predict.py:131-137``"
        vals, extra = _measure_pairs([self], [predictions], [test])
        return _scalar(extra[0]["sum"][0]), int(extra[0]["n"][0])

    def __call__(self, predictions: ItemList, test: ItemList | None = None) -> float:
        return self.extract_list_metrics(self.measure_list(predictions, test))

    def extract_list_metrics(self, data, /):
        val, n = data
        x = val / n if n else float("nan")
        return sqrt(x) if self._root else x

    def _check(self, p: dict):
        """
        The ``"error"`` dispositions as the reference's loop meets them (``predict.py:105-109``):
        the first list that has a missing value of a kind that is an error, and inside that list
        missing scores before missing truth.
        """
        ms = p["n_missing_score"] if self.missing_scores == "error" else np.zeros_like(p["n"])
        mt = p["n_missing_truth"] if self.missing_truth == "error" else np.zeros_like(p["n"])
        bad = np.flatnonzero((ms > 0) | (mt > 0))
        if len(bad):
            q = bad[0]
            if ms[q] > 0:
                raise ValueError(f"missing scores for {int(ms[q])} truth items")
            raise ValueError(f"missing truth for {int(mt[q])} scored items")

    def _compose_pred(self, p: dict):
        self._check(p)
        tot = p["sae"] if not self._root else p["sse"]
        n = p["n"]
        with np.errstate(divide="ignore", invalid="ignore"):
            x = tot / n
            if self._root:
                x = np.sqrt(x)
        return x, {"sum": tot, "n": n}

    def _summarize(self, values, extra) -> dict:
        "``AvgErrorAccumulator.accumulate`` (``predict.py:201-207``)"
        stats = _value_stats(values)
        tot, n = float(np.sum(extra["sum"])), int(np.sum(extra["n"]))
        x = tot / n if n else float("nan")
        return stats | {"global": sqrt(x) if self._root else x}


class RMSE(PredictMetric):
    "``predict.py:114-144``"

    _root = True


class MAE(PredictMetric):
    "``predict.py:147-176``"


def _scalar(x):
    return x.item() if isinstance(x, np.generic) else x


def _value_stats(values: np.ndarray) -> dict:
    "``ValueStatAccumulator.accumulate`` (data/accum/_value.py:57-64) over the non-NaN values"
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (mean of nothing, as the reference)
        return {"n": len(v), "mean": np.mean(v).item(), "median": np.median(v).item(),
                "std": np.std(v).item()}


# ---------------------------------------------------------------------------------------
# collections as arrays
# ---------------------------------------------------------------------------------------


class _Packed:
    """
    A collection's lists as arrays: ``dense`` = ([B x ld] item numbers, -1 padded, host array or
    device tensor; the vocabulary they number) or ``ragged`` = (int64 offsets, item ids, fields).
    """

    def __init__(self, keys, key_fields, *, dense=None, ragged=None, scores=None):
        self.keys, self.key_fields = keys, tuple(key_fields)
        self.dense, self.ragged, self.scores = dense, ragged, scores

    def __len__(self):
        return len(self.keys)

    def key_columns(self) -> dict[str, np.ndarray]:
        keys = self.keys
        if isinstance(keys, np.ndarray) and keys.ndim == 1 and len(self.key_fields) == 1:
            return {self.key_fields[0]: keys}
        if isinstance(keys, np.ndarray) and keys.ndim == 2:
            return {f: keys[:, j] for j, f in enumerate(self.key_fields)}
        rows = [k if isinstance(k, tuple) else (k,) for k in keys]
        return {f: np.asarray([r[j] for r in rows]) for j, f in enumerate(self.key_fields)}

    def as_ragged(self):
        """(offsets starting at 0, item ids or None, item numbers or None, vocabulary, fields):
        the arrays hold exactly the ``offsets[-1]`` entries of the lists"""
        if self.ragged is not None:
            offsets, ids, fields = self.ragged
            offsets = np.asarray(offsets, dtype=np.int64)
            lo, hi = int(offsets[0]), int(offsets[-1])
            return (offsets - lo, np.asarray(ids)[lo:hi], None, None,
                    {f: np.asarray(v)[lo:hi] for f, v in fields.items()})
        nums, vocab = self.dense
        nums = nums.cpu().numpy() if not isinstance(nums, np.ndarray) else nums
        keep = nums >= 0
        offsets = np.zeros(len(nums) + 1, np.int64)
        np.cumsum(keep.sum(axis=1), out=offsets[1:])
        fields = {}
        if self.scores is not None:
            sc = self.scores
            sc = sc.cpu().numpy() if not isinstance(sc, np.ndarray) else sc
            fields["score"] = sc[keep]
        return offsets, None, nums[keep], vocab, fields


def pack_collection(coll: ItemListCollection) -> _Packed:
    """
    The lists of a collection as arrays.  Array-backed collections (``from_arrays``,
    ``from_ragged``) hand over the arrays they hold -- no ``ItemList`` is built; a list-backed
    one is concatenated into ragged arrays (the fields every list carries).
    """
    ll = coll._lists
    if isinstance(ll, _RaggedLists) and not ll.extra:
        return _Packed(ll.raw_keys, coll.key_fields,
                       ragged=(ll.offsets, ll.item_ids, dict(ll.fields)))
    if isinstance(ll, _LazyLists) and not ll.extra:
        return _Packed(ll.raw_keys, coll.key_fields, dense=(ll.nums, ll.vocab), scores=ll.scores)
    keys, lists = [], []
    for key, il in ll:
        keys.append(tuple(key))
        lists.append(il)
    offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(il) for il in lists], out=offsets[1:])
    ids = [il.ids() for il in lists if len(il)]
    item_ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    common = None
    for il in lists:
        common = set(il._fields) if common is None else common & set(il._fields)
    fields = {f: (np.concatenate([il._fields[f] for il in lists if len(il)]) if ids
                  else np.zeros(0, np.float32)) for f in sorted(common or ())}
    return _Packed(keys, coll.key_fields, ragged=(offsets, item_ids, fields))


def dense_lists(packed: _Packed, vocab: Vocabulary) -> tuple[np.ndarray, Vocabulary]:
    """
    Ranked lists as one [B x L] int32 array of item numbers of ``vocab``, -1 padded at the end;
    an item ``vocab`` does not know keeps its place as :data:`UNKNOWN_ITEM`.
    """
    if packed.dense is not None:
        return packed.dense
    offsets, ids, _fields = packed.ragged
    lens = np.diff(offsets)
    B, L = len(lens), int(lens.max()) if len(lens) else 0
    out = np.full((B, L), -1, np.int32)
    if L:
        lo, hi = int(offsets[0]), int(offsets[-1])
        nums = vocab.numbers(ids[lo:hi], missing="negative") if hi > lo else np.zeros(0, np.int32)
        nums = np.where(nums < 0, UNKNOWN_ITEM, nums).astype(np.int32)
        col = np.arange(hi - lo) - np.repeat(offsets[:-1] - lo, lens)
        out[np.repeat(np.arange(B), lens), col] = nums
    return out, vocab


class TruthState:
    """
    A test collection as a CSR (test lists x item numbers; rows ascending, duplicate-free) on the
    host and -- per value field, uploaded once -- on the device.  ``lens`` are the test lists' own
    lengths (``len(test)`` counts every item, also a repeated one or one the vocabulary does not
    know: such ids are numbered past ``len(vocab)`` and can never be hit).
    """

    def __init__(self, coll: ItemListCollection, vocab: Vocabulary | None):
        p = pack_collection(coll)
        self.size = len(coll)
        self.key_fields = p.key_fields
        self.keys = p.key_columns()
        offsets, ids, nums, own_vocab, fields = p.as_ragged()
        self.lens = np.diff(offsets).astype(np.int64)
        self.extra_ids = None  # test ids the vocabulary does not know, ascending
        if nums is not None and (vocab is None or vocab is own_vocab or vocab == own_vocab):
            vocab = own_vocab
        else:
            if ids is None:
                ids = own_vocab.ids(nums)
            if vocab is None:
                vocab = Vocabulary(ids, "item")
            nums = vocab.numbers(ids, missing="negative") if len(ids) else np.zeros(0, np.int32)
            bad = nums < 0
            if bad.any():  # ids the vocabulary does not know: numbered past it
                extra, inv = np.unique(ids[bad], return_inverse=True)
                nums = nums.astype(np.int64)
                nums[bad] = len(vocab) + inv
                self.extra_ids = extra
        self.vocab = vocab
        self.n_cols = int(max(len(vocab), int(nums.max()) + 1 if len(nums) else 0))
        rows = np.repeat(np.arange(len(self.lens)), self.lens)
        order = np.lexsort((nums, rows))
        r, c = rows[order], np.asarray(nums)[order]
        first = np.ones(len(order), bool)
        first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
        self.src = order[first] + 0  # CSR entry -> position in the test arrays
        self.indices = c[first].astype(np.int32)
        self.indptr = np.zeros(len(self.lens) + 1, np.int64)
        np.cumsum(np.bincount(r[first], minlength=len(self.lens)), out=self.indptr[1:])
        self._fields = fields
        self._device: dict = {}
        self._index = None

    def values(self, field: str) -> np.ndarray:
        "``field`` per CSR entry (float32); test lists without any item need not carry it"
        if field not in self._fields:
            if len(self.src) == 0:  # len(test) == 0 answers before the field is looked at
                return np.zeros(0, np.float32)
            raise KeyError(f"test items have no field {field}")
        return np.asarray(self._fields[field])[self.src].astype(np.float32)

    def device_csr(self, field: str | None, dev):
        "the truth matrix in HBM with ``field`` as values (None: structure only), uploaded once"
        from . import _device as D

        hit = self._device.get((field, str(dev)))
        if hit is None:
            base = next((v for (f, d), v in self._device.items() if d == str(dev)), None)
            vals = None if field is None else self.values(field)
            if base is None:
                hit = D.DeviceCSR.from_arrays(self.indptr, self.indices,
                                              np.zeros(0, np.float32) if vals is None else vals,
                                              (len(self.lens), self.n_cols), dev)
                if vals is None:
                    hit.values = None
            else:  # (the structure is uploaded once; a further field adds its values)
                import torch

                hit = D.DeviceCSR(base.indptr, base.indices,
                                  None if vals is None else torch.from_numpy(vals).to(dev),
                                  base.shape, base.h_indptr)
            self._device[(field, str(dev))] = hit
        return hit

    def match(self, out_keys: dict[str, np.ndarray], n: int) -> np.ndarray:
        """
        Row of the test list of every output key, -1 without one: the output keys projected onto
        the test collection's key fields (``lookup_projected``); of equal test keys the last wins.
        """
        if self._index is None:
            self._index = key_index(self.key_fields, self.keys)
        return project_rows(self._index, self.key_fields, out_keys, n, "test")


def key_index(key_fields, keys: dict[str, np.ndarray]):
    "(index over a collection's keys, position of each index entry); of equal keys the last wins"
    cols = [keys[f] for f in key_fields]
    idx = pd.Index(cols[0]) if len(cols) == 1 else pd.MultiIndex.from_arrays(cols)
    pos = np.arange(len(idx))
    if not idx.is_unique:
        keep = ~idx.duplicated(keep="last")
        idx, pos = idx[keep], pos[keep]
    return idx, pos


def project_rows(index, key_fields, out_keys: dict[str, np.ndarray], n: int,
                 what: str = "test") -> np.ndarray:
    "row in the indexed collection of every output key projected onto its key fields, -1 = none"
    missing = [f for f in key_fields if f not in out_keys]
    if missing:
        raise KeyError(f"output keys lack the {what} key fields {missing}")
    idx, pos = index
    cols = [np.asarray(out_keys[f]) for f in key_fields]
    probe = cols[0] if len(cols) == 1 else pd.MultiIndex.from_arrays(cols)
    if len(idx) == 0:
        return np.full(n, -1, np.int32)
    loc = idx.get_indexer(probe)
    return np.where(loc >= 0, pos[np.maximum(loc, 0)], -1).astype(np.int32)


_TRUTH: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def truth_state(test: ItemListCollection, vocab: Vocabulary | None = None) -> TruthState:
    """
    The :class:`TruthState` of a test collection, built once per (collection, vocabulary) and
    kept while the collection lives and has the same number of lists.  A test collection is
    taken to be fixed once it has been measured against: lists replaced, or arrays changed in
    place, with the count unchanged are NOT noticed (``_TRUTH.pop(test, None)`` forgets it).
    """
    per = _TRUTH.setdefault(test, {})
    key = None if vocab is None else id(vocab)
    hit = per.get(key)
    if hit is None or hit[0].size != len(test) or (vocab is not None and hit[1] is not vocab):
        hit = per[key] = (TruthState(test, vocab), vocab)
    return hit[0]


# ---------------------------------------------------------------------------------------
# the batched pass
# ---------------------------------------------------------------------------------------


class _RankPlan:
    "What the ranking metrics of one call need: cutoffs, weight tables, gain fields, ideals."

    def __init__(self):
        self.cutoffs: list[int] = []  # kernel cutoffs: 0 = whole list
        self.weights: dict = {}  # table key -> (row, RankWeight)
        self.gains: list[str] = []
        self.ideals: list[tuple] = []  # (cutoff, table key, gain)

    def need(self, n, weight: RankWeight | None = None, gain: str | None = None, ideal=False):
        c = 0 if n is None else int(n)
        if n != 0 and c not in self.cutoffs:
            self.cutoffs.append(c)
        if weight is not None and weight._table_key() not in self.weights:
            self.weights[weight._table_key()] = (len(self.weights), weight)
        if gain is not None and gain not in self.gains:
            self.gains.append(gain)
        if ideal and n != 0 and (c, weight._table_key(), gain) not in self.ideals:
            self.ideals.append((c, weight._table_key(), gain))


class _RankStats:
    "The kernels' statistics of one batch on the host, by cutoff / weight / gain field."

    def __init__(self, B, n_test, tables):
        self.B, self.n_test, self.tables = B, n_test, tables  # tables: key -> float64 [Lmax]
        self.n_recs_all = np.zeros(B, np.int64)
        self.ints: dict = {}
        self.sums: dict = {}
        self.counts: dict = {}
        self.ideals: dict = {}

    def _zero(self):
        return np.zeros(self.B)

    def n_recs(self, n):
        return self.n_recs_all if n is None else np.minimum(self.n_recs_all, n)

    def n_hits(self, n):
        return np.zeros(self.B, np.int64) if n == 0 else self.ints[(n or 0, "hits")]

    def first_hit(self, n):
        return np.zeros(self.B, np.int64) if n == 0 else self.ints[(n or 0, "first")]

    def ap_sum(self, n):
        return self._zero() if n == 0 else self.sums[(n or 0, "ap", None, None)]

    def w_hits(self, n, weight):
        return self._zero() if n == 0 else self.sums[(n or 0, "w", weight._table_key(), None)]

    def g_hits(self, n, weight, gain):
        return self._zero() if n == 0 else self.sums[(n or 0, "g", weight._table_key(), gain)]

    def gain_count(self, gain):
        return self.counts[gain]

    def ideal(self, n, weight, gain):
        return self._zero() if n == 0 else self.ideals[(n or 0, weight._table_key(), gain)]

    def prefix(self, weight, counts) -> np.ndarray:
        "``np.sum(weight.weight(arange(1, c + 1)))`` per entry of ``counts`` (``fixed_dcg``)"
        w = self.tables[weight._table_key()]
        u, inv = np.unique(counts, return_inverse=True)
        vals = np.array([np.sum(w[:c]).item() for c in u], dtype=np.float64)
        return vals[inv] if len(u) else np.zeros(0)


def _sync(timing):
    if timing is not None:
        import torch

        torch.cuda.synchronize()


def _rank_pass(metrics, lists, vocab_truth: TruthState | None, rows, n_test, dev, timing=None):
    """
    ``lists``: device int32 [B x ld].  Gathers the lists' truth rows, runs lk_rank_stats (one
    launch per group of cutoffs / tables that fits a wave, per gain field) and lk_ideal_gain, and
    returns the statistics on the host.
    """
    import time

    import torch

    from . import _device as D

    plan = _RankPlan()
    for m in metrics:
        m._request(plan)
    B, ld = int(lists.shape[0]), int(lists.shape[1])
    t0 = time.perf_counter()
    fields = plan.gains or [None]
    if vocab_truth is None:  # no test data at all: every row is empty
        empty = D.DeviceCSR(torch.zeros(B + 1, dtype=torch.int64, device=dev),
                            torch.empty(0, dtype=torch.int32, device=dev),
                            torch.empty(0, dtype=torch.float32, device=dev), (B, 1),
                            np.zeros(B + 1, np.int64))
        truths = {f: empty for f in fields}
    else:
        truths = {f: D.gather_rows(vocab_truth.device_csr(f, dev), rows,
                                   with_values=f is not None) for f in fields}
    _sync(timing)
    t1 = time.perf_counter()
    first = truths[fields[0]]
    longest = int(np.diff(first.h_indptr).max()) if B else 0
    lmax = max(ld, int(n_test.max()) if B else 0, longest, 1)
    ranks = np.arange(1, lmax + 1)
    keys = list(plan.weights)
    tables = {k: np.ascontiguousarray(plan.weights[k][1].weight(ranks), dtype=np.float64)
              for k in keys}
    stats = _RankStats(B, n_test, tables)
    W = torch.from_numpy(np.stack([tables[k] for k in keys])).to(dev) if keys else None
    cutoffs = plan.cutoffs or [0]
    pending = []
    for fi, f in enumerate(fields):
        for ta in range(0, max(len(keys), 1), D.RANK_STATS_MAX_TABLES):
            tk = keys[ta:ta + D.RANK_STATS_MAX_TABLES]
            step = min(D.RANK_STATS_MAX_CUTOFFS, 64 // (1 + 2 * len(tk)))
            for ca in range(0, len(cutoffs), step):
                cs = cutoffs[ca:ca + step]
                cnt, sm = D.rank_stats(lists, truths[f], cs,
                                       None if not tk else W[ta:ta + len(tk)].contiguous(),
                                       gains=f is not None)
                pending.append((fi, f, tk, cs, cnt, sm))
    ideal_pending = []
    for f in plan.gains:
        combos = [(c, keys.index(k)) for (c, k, g) in plan.ideals if g == f] or [(0, 0)]
        names = [(c, k) for (c, k, g) in plan.ideals if g == f]
        if W is None:
            raise ValueError("graded metrics need a rank weight")
        if truths[f].nnz == 0:  # every truth row is empty: no gain exists, every value is NaN
            stats.counts[f] = np.zeros(B, np.int64)
            for c, k in names:
                stats.ideals[(c, k, f)] = np.zeros(B)
            continue
        for a in range(0, len(combos), D.RANK_STATS_MAX_CUTOFFS):
            ideal, count = D.ideal_gain(truths[f], combos[a:a + D.RANK_STATS_MAX_CUTOFFS], W)
            ideal_pending.append((f, names[a:a + D.RANK_STATS_MAX_CUTOFFS], ideal, count))
    _sync(timing)
    t2 = time.perf_counter()
    for fi, f, tk, cs, cnt, sm in pending:
        cnt, sm = cnt.cpu().numpy(), sm.cpu().numpy()
        per = 1 + 2 * len(tk)
        if fi == 0:
            stats.n_recs_all = cnt[0].astype(np.int64)
        for j, c in enumerate(cs):
            if fi == 0:
                stats.ints[(c, "hits")] = cnt[2 + 2 * j].astype(np.int64)
                stats.ints[(c, "first")] = cnt[3 + 2 * j].astype(np.int64)
                stats.sums[(c, "ap", None, None)] = sm[j * per]
            for t, k in enumerate(tk):
                if fi == 0:
                    stats.sums[(c, "w", k, None)] = sm[j * per + 1 + 2 * t]
                if f is not None:
                    stats.sums[(c, "g", k, f)] = sm[j * per + 2 + 2 * t]
    for f, names, ideal, count in ideal_pending:
        ideal = ideal.cpu().numpy()
        stats.counts[f] = count.cpu().numpy().astype(np.int64)
        for j, (c, k) in enumerate(names):
            stats.ideals[(c, k, f)] = ideal[j]
    if timing is not None:
        timing["gather_s"] = timing.get("gather_s", 0.0) + (t1 - t0)
        timing["kernel_s"] = timing.get("kernel_s", 0.0) + (t2 - t1)
        timing["download_s"] = timing.get("download_s", 0.0) + (time.perf_counter() - t2)
    return stats


def _predict_pass(packed: _Packed, truth: TruthState | None, rows, dev, timing=None) -> dict:
    "lk_predict_errors over the lists of ``packed`` (ragged, with a ``score`` field)"
    import time

    import torch

    from . import _device as D

    offsets, ids, nums, vocab, fields = packed.as_ragged()
    if "score" not in fields:
        raise AssertionError("item list does not have scores")
    ptr = np.ascontiguousarray(offsets, dtype=np.int64)
    scores = np.ascontiguousarray(fields["score"], dtype=np.float32)
    if truth is None and "rating" not in fields:
        raise AssertionError("no ratings provided")
    if len(scores) == 0 and truth is None:  # (nothing to launch over)
        z = np.zeros(len(ptr) - 1, np.int64)
        return {"sse": z.astype(np.float64), "sae": z.astype(np.float64), "n": z,
                "n_missing_score": z, "n_missing_truth": z}
    t0 = time.perf_counter()
    d_ptr = torch.from_numpy(ptr).to(dev)
    d_scores = torch.from_numpy(scores).to(dev)
    if truth is None:
        own = np.ascontiguousarray(fields["rating"], dtype=np.float32)
        sums, counts = D.predict_errors(d_ptr, None, d_scores, None, torch.from_numpy(own).to(dev))
    else:
        if nums is None:
            nums = truth.vocab.numbers(ids, missing="negative") if len(ids) else \
                np.zeros(0, np.int32)
            extra = truth.extra_ids
            if extra is not None and (nums < 0).any():
                bad = np.flatnonzero(nums < 0)
                at = np.searchsorted(extra, ids[bad])
                ok = (at < len(extra)) & (extra[np.minimum(at, len(extra) - 1)] == ids[bad])
                nums = nums.copy()
                nums[bad[ok]] = len(truth.vocab) + at[ok]
        elif not (vocab is truth.vocab or vocab == truth.vocab):
            nums = truth.vocab.numbers(vocab.ids(nums), missing="negative")
        t = D.gather_rows(truth.device_csr("rating", dev), rows)
        d_nums = torch.from_numpy(np.ascontiguousarray(nums, dtype=np.int32)).to(dev)
        sums, counts = D.predict_errors(d_ptr, d_nums, d_scores, t)
    _sync(timing)
    t1 = time.perf_counter()
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    if timing is not None:
        timing["kernel_s"] = timing.get("kernel_s", 0.0) + (t1 - t0)
    return {"sse": sums[0], "sae": sums[1], "n": counts[0], "n_missing_score": counts[1],
            "n_missing_truth": counts[2]}


class _ListPass:
    """
    The lists of one batch on the device, numbered by the vocabulary a metric asks for, with the
    rank-weight tables: a dense panel is uploaded once and shared by every metric (renumbered on
    the device for a metric whose vocabulary is another one); ragged lists are numbered on the
    host once per vocabulary.
    """

    def __init__(self, packed: _Packed, dev, state: dict):
        self.packed, self.dev, self.state = packed, dev, state
        self._lists: list = []  # (vocabulary, device int32 [B x L])
        self._tables: dict = {}

    def zeros(self, n: int):
        import torch

        return torch.zeros(n, dtype=torch.float64, device=self.dev)

    def _upload(self, nums):
        import torch

        if isinstance(nums, np.ndarray):
            nums = torch.from_numpy(np.ascontiguousarray(nums, dtype=np.int32)).to(self.dev)
        return nums.contiguous()

    def lists(self, vocab: Vocabulary):
        import torch

        for v, t in self._lists:
            if v is vocab or v == vocab:
                return t
        if self.packed.dense is not None:
            if not self._lists:
                nums, own = self.packed.dense
                self._lists.append((own, self._upload(nums)))
                return self.lists(vocab)
            own, panel = self._lists[0]
            to = vocab.numbers(own.ids(), missing="negative") if len(own) else \
                np.zeros(0, np.int32)
            to = self._upload(np.append(np.where(to < 0, UNKNOWN_ITEM, to), UNKNOWN_ITEM))
            at = torch.clamp(panel, min=0, max=len(own)).to(torch.int64)
            t = torch.where(panel >= 0, to[at], panel).contiguous()
        else:
            t = self._upload(dense_lists(self.packed, vocab)[0])
        self._lists.append((vocab, t))
        return t

    def table(self, weight: RankWeight):
        "``weight``'s table over the ranks of the batch's lists (device float64 [L])"
        L = max(int(self._lists[0][1].shape[1]), 1)
        hit = self._tables.get(weight._table_key())
        if hit is None:
            w = np.ascontiguousarray(weight.weight(np.arange(1, L + 1)), dtype=np.float64)
            hit = self._tables[weight._table_key()] = _to_dev(w, self.dev)
        return hit


def measure_arrays(metrics, packed: _Packed, test: ItemListCollection | None, *, outputs=None,
                   timing: dict | None = None, state: dict | None = None):
    """
    Every metric of ``metrics`` for every list of ``packed`` in one batched pass.  Returns
    (values: one float64 [B] array per metric -- None for a metric without per-list values --,
    extras: per metric None or the prediction metrics' {"sum", "n"} arrays, number of lists
    without test data).  ``state``: the collector's device state of the metrics that accumulate
    over a run (the Gini totals), by ``id(metric)``.
    """
    import time

    from . import _device as D

    dev = D.device()
    B = len(packed)
    rank_ms = [m for m in metrics if m._kind == "rank"]
    pred_ms = [m for m in metrics if m._kind == "predict"]
    func_ms = [m for m in metrics if m._kind == "function"]
    list_ms = [m for m in metrics if m._kind == "lists"]
    dlists = _ListPass(packed, dev, {} if state is None else state)
    t0 = time.perf_counter()
    truth = rows = None
    n_test = np.zeros(B, np.int64)
    if test is not None:
        vocab = packed.dense[1] if packed.dense is not None else None
        truth = truth_state(test, vocab)
        rows = truth.match(packed.key_columns(), B)
        n_test = np.where(rows >= 0, truth.lens[np.maximum(rows, 0)], 0) if truth.size else n_test
    no_test = int((rows < 0).sum()) if rows is not None else 0
    if timing is not None:
        timing["match_s"] = timing.get("match_s", 0.0) + (time.perf_counter() - t0)
    values: dict[int, Any] = {}
    extras: dict[int, Any] = {}
    if rank_ms:
        if test is None:
            raise TypeError("ranking metrics need test data")
        stats = _rank_pass(rank_ms, dlists.lists(truth.vocab), truth if truth.size else None,
                           rows, n_test, dev, timing)
        t1 = time.perf_counter()
        for m in rank_ms:
            values[id(m)] = np.asarray(m._compose(stats), dtype=np.float64)
        empty = int(((n_test == 0) & (rows >= 0)).sum())
        if empty and any(getattr(m, "_warns_empty", False) for m in rank_ms):
            warnings.warn(f"test item list is empty for {empty} lists", DataWarning, stacklevel=3)
        if timing is not None:
            timing["compose_s"] = timing.get("compose_s", 0.0) + (time.perf_counter() - t1)
    if list_ms:
        t1 = time.perf_counter()
        pending = [m._launch(dlists) for m in list_ms]
        _sync(timing)
        t2 = time.perf_counter()
        for m, pend in zip(list_ms, pending):
            values[id(m)] = m._finish(pend, B)
        if timing is not None:
            timing["kernel_s"] = timing.get("kernel_s", 0.0) + (t2 - t1)
            timing["download_s"] = timing.get("download_s", 0.0) + (time.perf_counter() - t2)
    if pred_ms:
        p = _predict_pass(packed, truth if test is not None else None, rows, dev, timing)
        for m in pred_ms:
            values[id(m)], extras[id(m)] = m._compose_pred(p)
    if func_ms:
        if outputs is None:
            raise TypeError("function metrics run list by list and need the collection itself")
        none = ItemList([])
        for m in func_ms:
            vals = np.empty(B)
            for i, (_key, il) in enumerate(outputs):
                tl = test._lists[int(rows[i])][1] if rows is not None and rows[i] >= 0 else none
                v = m.measure_list(il, tl)
                vals[i] = np.nan if v is None else v
            values[id(m)] = vals
    return [values[id(m)] for m in metrics], [extras.get(id(m)) for m in metrics], no_test


def _measure_pairs(metrics, outputs: list, tests: list, state: dict | None = None):
    "``measure_list``: the batched pass over a batch built from the given pairs"
    out = ItemListCollection(("list",))
    for i, il in enumerate(outputs):
        out.add(il, i)
    test = None
    if any(t is not None for t in tests):
        test = ItemListCollection(("list",))
        for i, il in enumerate(tests):
            test.add(il if il is not None else ItemList([]), i)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DataWarning)
        vals, extras, _ = measure_arrays(metrics, pack_collection(out), test, outputs=out,
                                         state=state)
    return vals, extras


# ---------------------------------------------------------------------------------------
# collector (``_collect.py``) and run analysis (``bulk.py``)
# ---------------------------------------------------------------------------------------


class RunMetrics(NamedTuple):
    "``_collect.py:30-42``"

    summary_metrics: dict
    list_metrics: pd.DataFrame


def _wrap_metric(m) -> Metric:
    if isinstance(m, type):
        m = m()
    elif not isinstance(m, Metric):
        m = FunctionMetric(m)
    return m


def _add_values(record: dict, name: str, data):
    if data is None:
        return
    if isinstance(data, dict):
        for k, v in data.items():
            record[f"{name}.{k}"] = v
    else:
        record[name] = data


class MeasurementCollector:
    """
    ``lenskit.metrics.MeasurementCollector`` (``_collect.py:60-245``).  The test collection's
    device form is built at its first use and kept with the collection (:func:`truth_state`): a
    test collection must not be changed once it has been measured against.  Measurements arrive a
    batch at a time: :meth:`add_collection_measurements` runs every metric over every list of a
    collection in one device pass (array-backed collections are not turned into lists), and
    :meth:`add_array_measurements` takes the result arrays of a batched recommend call as they
    are -- device tensors included, which then never visit the host.
    """

    def __init__(self):
        self._metrics: list[tuple[str, Metric]] = []
        self._chunks: list[tuple[dict, list, list]] = []  # key columns, values, extras
        self._state: dict = {}  # id(metric) -> device state kept over the add_* calls (Gini totals)
        self.key_fields: list[str] = []

    def empty_copy(self):
        copy = MeasurementCollector()
        copy._metrics = list(self._metrics)
        return copy

    def reset(self):
        self.key_fields = []
        self._chunks = []
        self._state = {}

    @property
    def metric_names(self) -> list[str]:
        return [label for label, _m in self._metrics]

    def add_metric(self, metric, label: str | None = None):
        m = _wrap_metric(metric)
        label = m.label if label is None else label
        if label in self.metric_names:
            raise RuntimeError(f"duplicate metric: {label}")
        self._metrics.append((label, m))

    def _validate_setup(self):
        seen = set()
        for lbl in self.metric_names:
            if lbl in seen:
                raise RuntimeError(f"duplicate metric: {lbl}")
            seen.add(lbl)

    def _record(self, key_cols: dict, vals, extras):
        if not self.key_fields:
            self.key_fields = list(key_cols)
        self._chunks.append((key_cols, vals, extras))

    def add_list_measurement(self, output: ItemList, test: ItemList, **keys: Any):
        ms = [m for _l, m in self._metrics]
        vals, extras = _measure_pairs(ms, [output], [test], self._state)
        self._record({k: np.asarray([v]) for k, v in keys.items()}, vals, extras)

    def _add_packed(self, packed: _Packed, test, keys: dict, outputs=None, timing=None):
        ms = [m for _l, m in self._metrics]
        vals, extras, no_test = measure_arrays(ms, packed, test, outputs=outputs, timing=timing,
                                               state=self._state)
        cols = {k: np.full(len(packed), v) for k, v in keys.items()}
        cols.update(packed.key_columns())
        self._record(cols, vals, extras)
        if no_test:
            _log.warning("could not find test data for %d lists", no_test)

    def add_collection_measurements(self, outputs: ItemListCollection, test: ItemListCollection,
                                    *, timing: dict | None = None, **keys: Any):
        _log.debug("measuring %d metrics for %d output lists", len(self._metrics), len(outputs))
        self._add_packed(pack_collection(outputs), test, keys, outputs=outputs, timing=timing)

    def add_array_measurements(self, keys, item_nums, test: ItemListCollection, *,
                               vocabulary: Vocabulary, scores=None, key=("user_id",),
                               timing: dict | None = None, **more_keys: Any):
        """
        Measure the [B x n] item numbers (-1 padded) of a batched recommend call against ``test``:
        host arrays or the device tensors of ``recommend_batch(..., device_output=True)`` with
        the keys (``keys[i]`` is row ``i``'s key) and the vocabulary the numbers belong to.
        """
        key = (key,) if isinstance(key, str) else tuple(key)
        packed = _Packed(keys if isinstance(keys, np.ndarray) else list(keys), key,
                         dense=(item_nums, vocabulary), scores=scores)
        self._add_packed(packed, test, more_keys, timing=timing)

    def measure_run(self, outputs: ItemListCollection, test: ItemListCollection) -> RunMetrics:
        copy = self.empty_copy()
        copy.add_collection_measurements(outputs, test)
        return RunMetrics(copy.summary_metrics(), copy.list_metrics())

    def _column(self, j: int) -> np.ndarray:
        parts = [vals[j] for _k, vals, _e in self._chunks]
        return np.concatenate(parts) if parts else np.zeros(0)

    def list_metrics(self) -> pd.DataFrame:
        cols = {}
        for f in self.key_fields:
            cols[f] = np.concatenate([k[f] for k, _v, _e in self._chunks])
        for j, (label, m) in enumerate(self._metrics):
            if not hasattr(m, "_summarize_state"):  # (a metric without per-list values)
                cols[label] = self._column(j)
        df = pd.DataFrame(cols)
        if self.key_fields:
            df.set_index(self.key_fields, inplace=True, drop=True)
        return df

    def summary_metrics(self) -> dict:
        results: dict = {}
        for j, (label, m) in enumerate(self._metrics):
            if hasattr(m, "_summarize_state"):
                _add_values(results, label, m._summarize_state(self._state.get(id(m))))
                continue
            ex = [e[j] for _k, _v, e in self._chunks if e[j] is not None]
            extra = {k: np.concatenate([e[k] for e in ex]) for k in ex[0]} if ex else \
                {"sum": np.zeros(0), "n": np.zeros(0, np.int64)}
            _add_values(results, label, m._summarize(self._column(j), extra))
        return results


class RunAnalysisResult:
    """``bulk.py:26-115``.  ``outputs`` (not in the reference): what the measured run produced,
    when the producer keeps it -- :func:`quick_measure_model` stores its ``split``,
    ``recommendations`` and ``predictions`` there; None otherwise."""

    def __init__(self, lmvs: pd.DataFrame, gmvs: pd.Series, defaults: dict,
                 outputs: dict | None = None):
        self._list_metrics = lmvs
        self._global_metrics = gmvs
        self._defaults = defaults
        self.outputs = outputs

    def global_metrics(self) -> pd.Series:
        return self._global_metrics

    def list_metrics(self, fill_missing=True) -> pd.DataFrame:
        if fill_missing:
            return self._list_metrics.fillna(self._defaults)
        return self._list_metrics

    def list_summary(self, *keys: str) -> pd.DataFrame:
        scores = self.list_metrics(fill_missing=True)
        if keys:
            df = scores.groupby(list(keys)).agg(["mean", "median", "std"]).stack(level=0)
        else:
            df = scores.agg(["mean", "median", "std"]).T
            df.index.name = "metric"
        return df

    def merge_from(self, other: "RunAnalysisResult"):
        for c in self._list_metrics.columns:
            if c in other._list_metrics.columns:
                warnings.warn(f"list metric {c} appears in both merged results", DataWarning)
        for c in self._global_metrics.index:
            if c in other._global_metrics.index:
                warnings.warn(f"global metric {c} appears in both merged results", DataWarning)
        self._list_metrics = self._list_metrics.join(other._list_metrics, how="outer")
        self._global_metrics = pd.concat([self._global_metrics, other._global_metrics])
        self._defaults = self._defaults | other._defaults


class RunAnalysis:
    "``bulk.py:118-210`` (kept for the reference's callers; the collector is the interface)"

    def __init__(self, *metrics):
        self.collector = MeasurementCollector()
        self._defaults: dict = {}
        for metric in metrics:
            self.add_metric(metric)

    def add_metric(self, metric, label: str | None = None, default: float | None = None):
        self.collector.add_metric(metric, label)
        if default is not None:
            self._defaults[self.collector._metrics[-1][0]] = default

    def compute(self, outputs, test) -> RunAnalysisResult:
        return self.measure(outputs, test)

    def measure(self, outputs, test) -> RunAnalysisResult:
        copy = self.collector.empty_copy()
        copy._validate_setup()
        copy.add_collection_measurements(outputs, test)
        return RunAnalysisResult(copy.list_metrics(), pd.Series(copy.summary_metrics()),
                                 dict(self._defaults))


def quick_measure_model(model, data, *, predicts_ratings: bool = False, rng=None):
    """
    ``_quick.py:22-78``: hold out 20 % of the rows of a fifth of the users, train, recommend 20
    items per test user (and predict the held-out pairs), measure RecipRank / RBP / NDCG / Hit /
    Recall (and RMSE / MAE).
    """
    from . import batch
    from .pipeline import predict_pipeline, topn_pipeline
    from .splitting import SampleFrac, sample_users
    from .training import TrainingOptions

    pipe = predict_pipeline(model) if predicts_ratings else topn_pipeline(model)
    us_size = data.user_count // 5
    split = sample_users(data, us_size, SampleFrac(0.2, rng=rng), rng=rng)
    _log.info("measuring %s on %d users", model, us_size)
    pipe.train(split.train, TrainingOptions())
    users = pack_collection(split.test).key_columns()["user_id"]
    recs = batch.recommend(pipe, users, 20)
    rra = RunAnalysis()
    for m in (RecipRank(), RBP(), NDCG(), Hit(), Recall()):
        rra.add_metric(m)
    result = rra.measure(recs, split.test)
    if predicts_ratings:
        preds = batch.predict(pipe, split.test)
        pra = RunAnalysis()
        pra.add_metric(RMSE())
        pra.add_metric(MAE())
        result.merge_from(pra.measure(preds, split.test))
    result.outputs = {"split": split, "recommendations": recs,
                      "predictions": preds if predicts_ratings else None}
    return result
