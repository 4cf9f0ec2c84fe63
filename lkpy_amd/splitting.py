"""
Train / test splitting by user: ``lenskit.splitting`` (src/lenskit/splitting/_users.py,
``_holdout.py``, ``_split.py``), host NumPy.

The generator is drawn from **in the reference's order** -- ``sample_users``: one
``rng.choice(users, size, replace=False)`` (``_users.py:160``), then one ``method(row)`` per test
user in that order (``_users.py:184-188``), each ``SampleN`` / ``SampleFrac`` one
``rng.choice(len(row), n, replace=False)`` (``_holdout.py:69,96``); ``crossfold_users``:
``rng.shuffle(arange(n_users))`` + ``np.array_split`` (``_users.py:66-70``) -- so that a seed is
meant to give the split the reference gives.  No test pins that: the reference has not been run
next to this module, the claim rests on the line-by-line correspondence alone.

``test`` is a ragged-array ``ItemListCollection`` keyed by ``user_id`` whose lists carry the rows'
fields (``rating``, ...); ``train`` is a ``Dataset`` without the test pairs and with the
vocabularies of ``data`` (as ``DatasetBuilder(data)`` keeps them, ``_users.py:191-199``).
"""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Iterator

import numpy as np
import pandas as pd

from .data import Dataset, ItemList, ItemListCollection

_log = logging.getLogger(__name__)


def _generator(rng) -> np.random.Generator:
    "``random_generator`` (src/lenskit/random.py:181-185)"
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


class HoldoutMethod:
    "Picks the test rows of one user (``_holdout.py:19-41``)."

    def select(self, n: int, field) -> np.ndarray:
        "positions of the test rows among a user's ``n`` rows; ``field(name)`` gives a column"
        raise NotImplementedError()

    def __call__(self, items: ItemList) -> ItemList:
        return items[self.select(len(items), items.field)]


class SampleN(HoldoutMethod):
    "``_holdout.py:44-70``"

    def __init__(self, n: int, rng=None):
        self.n = n
        self.rng = _generator(rng)

    def select(self, n, field):
        if n <= self.n:
            return np.arange(n)
        return self.rng.choice(n, self.n, replace=False)


class SampleFrac(HoldoutMethod):
    "``_holdout.py:73-97``"

    def __init__(self, frac: float, rng=None):
        self.fraction = frac
        self.rng = _generator(rng)

    def select(self, n, field):
        return self.rng.choice(n, round(n * self.fraction), replace=False)


def _ordering(field, name):
    col = field(name)
    if col is None:
        raise TypeError(f"item list does not have ordering field {name}")
    return np.argsort(col)


class LastN(HoldoutMethod):
    "``_holdout.py:100-128``"

    def __init__(self, n: int, field: str = "timestamp"):
        self.n = n
        self.field = field

    def select(self, n, field):
        if n <= self.n:
            return np.arange(n)
        return _ordering(field, self.field)[-self.n:]


class LastFrac(HoldoutMethod):
    "``_holdout.py:131-156``"

    def __init__(self, frac: float, field: str = "timestamp"):
        self.fraction = frac
        self.field = field

    def select(self, n, field):
        k = round(n * self.fraction)
        return _ordering(field, self.field)[-k:]  # (k = 0: ``[-0:]`` is everything, as there)


@dataclass
class TTSplit:
    "``_split.py:22-90``"

    train: Dataset
    test: ItemListCollection
    name: str | None = None

    @property
    def test_size(self) -> int:
        return self.test.total_items()

    @property
    def test_df(self) -> pd.DataFrame:
        return self.test.to_df()

    @property
    def train_df(self) -> pd.DataFrame:
        ds = self.train
        df = pd.DataFrame({"user_id": ds.users.ids(ds._rows), "item_id": ds.items.ids(ds._cols)})
        for k, v in ds._attrs.items():
            df[k] = v
        return df


def _make_split(data: Dataset, test_us, method: HoldoutMethod, *, test_only=False) -> TTSplit:
    "``_users.py:172-199``"
    test_us = np.asarray(test_us)
    unums = data.users.numbers(test_us)
    picked, offsets = [], np.zeros(len(test_us) + 1, np.int64)
    for i, u in enumerate(unums):  # one ``method(row)`` per test user, in order
        s, e = int(data._indptr[u]), int(data._indptr[u + 1])
        sel = np.asarray(method.select(e - s, lambda f, s=s, e=e: None if f not in data._attrs
                                       else data._attrs[f][s:e]), dtype=np.int64)
        picked.append(s + sel)
        offsets[i + 1] = offsets[i] + len(sel)
    pos = np.concatenate(picked) if picked else np.zeros(0, np.int64)
    test = ItemListCollection.from_ragged(test_us, offsets, data.items.ids(data._cols[pos]),
                                          {k: v[pos] for k, v in data._attrs.items()},
                                          key=("user_id",))
    if test_only:
        keep = np.zeros(data.interaction_count, bool)
    else:  # every interaction of a test (user, item) pair leaves (``filter_interactions``)
        pair = data._rows.astype(np.int64) * max(data.item_count, 1) + data._cols
        keep = ~np.isin(pair, pair[pos])
    train = Dataset(data.users, data.items, data._rows[keep], data._cols[keep],
                    {k: v[keep] for k, v in data._attrs.items()})
    train.item_attrs = dict(data.item_attrs)  # (the items, and what is known of them, stay)
    return TTSplit(train, test)


def crossfold_users(data: Dataset, partitions: int, method: HoldoutMethod, *,
                    test_only: bool = False, rng=None) -> Iterator[TTSplit]:
    "``_users.py:27-81``: the users shuffled and cut into ``partitions`` test sets"
    rng = _generator(rng)
    users = data.users.ids()
    rows = np.arange(len(users))
    rng.shuffle(rows)
    for ts in np.array_split(rows, partitions):
        yield _make_split(data, users[ts], method, test_only=test_only)


def sample_users(data: Dataset, size: int, method: HoldoutMethod, *, repeats: int | None = None,
                 disjoint: bool = True, test_only: bool = False, rng=None):
    "``_users.py:106-169``: one split (``repeats=None``) or an iterator of ``repeats`` splits"
    rng = _generator(rng)
    users = data.users.ids()
    unums = np.arange(len(users))
    if disjoint and repeats is not None and repeats * size >= len(users):
        _log.warning("cannot take %d disjoint samples of size %d from %d users", repeats, size,
                     len(users))
        return crossfold_users(data, repeats, method)
    if repeats is None:
        test_us = rng.choice(users, size, replace=False)
        return _make_split(data, test_us, method)
    if disjoint:
        rng.shuffle(unums)
        test_usets = [unums[i * size:(i + 1) * size] for i in range(repeats)]
    else:
        test_usets = [rng.choice(len(users), size, replace=False) for _i in range(repeats)]
    return (_make_split(data, users[us], method, test_only=test_only) for us in test_usets)
