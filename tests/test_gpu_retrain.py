"""
GPU: the batched paths after a retrain.  A pipeline trained on ml-latest-small and
used through ``batch.recommend`` / ``batch.predict`` holds device state built from that data;
after ``Pipeline.train`` on a second, seeded synthetic dataset over the same items -- and after
retraining only the history lookup -- ``recommend_batch`` over a ``HistoryBatch``, the list path
and the per-query ``pipe.run`` must agree (item numbers, score bits), and ``batch.predict`` must
equal the per-query ``rating-predictor`` composition bit for bit.
"""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _synthetic(ml_ds, seed=5, n_users=400, nnz=24_000):
    "other users and interactions over ml-latest-small's item vocabulary"
    from lkpy_amd.data import Dataset

    rng = np.random.default_rng(seed)
    items = ml_ds.items.ids()
    pop = 1.0 / (rng.permutation(len(items)) + 10.0)  # a long-tailed popularity
    cells = np.unique(rng.integers(0, n_users, nnz) * len(items) +
                      rng.choice(len(items), nnz, p=pop / pop.sum()))
    ratings = rng.integers(1, 11, len(cells)) * 0.5
    ds = Dataset.from_arrays(cells // len(items) + 5_000_000, items[cells % len(items)], ratings,
                             all_item_ids=items)
    assert ds.items == ml_ds.items and ds.users != ml_ds.users
    return ds


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_recommend(pipe, users, n=10):
    from lkpy_amd import batch
    from lkpy_amd.data import RecQuery

    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    gi, gs = scorer.recommend_batch(lookup.batch(users), n)
    li, ls = scorer.recommend_batch([lookup(RecQuery.create(u)) for u in users], n)
    assert np.array_equal(gi, li)
    assert np.array_equal(_bits(gs), _bits(ls))
    assert (gi[-1] == -1).all()  # the unknown user
    out = batch.recommend(pipe, users, n)
    for pos, u in enumerate(users):
        listed = out.lookup(u).numbers(vocabulary=scorer.items)
        assert np.array_equal(listed, gi[pos][gi[pos] >= 0]), u
    for pos in range(0, len(users), 5):
        one = pipe.run("recommender", query=users[pos], n=n)
        keep = gi[pos] >= 0
        ws = np.asarray(one.scores(), np.float32)
        assert np.array_equal(_bits(ws), _bits(gs[pos][keep])), users[pos]
        wi = one.numbers(vocabulary=scorer.items)
        for j in np.flatnonzero(wi != gi[pos][keep]):
            # equal scores of different items may be listed in another order
            assert (ws == ws[j]).sum() > 1 or ws[j] == ws[-1], (users[pos], j)


def _check_predict(pipe, ds, users):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(len(users))
    items = ds.items.ids()
    pairs = {u: ItemList(np.concatenate([rng.choice(items, 25, replace=False), [10**9]]))
             for u in users}
    got = batch.predict(pipe, pairs)
    for u, il in pairs.items():
        want = pipe.run("rating-predictor", query=u, items=il)
        g = got.lookup(u)
        assert np.array_equal(g.ids(), want.ids()), u
        assert np.array_equal(_bits(g.scores()), _bits(want.scores())), u
        assert sorted(g._fields) == sorted(want._fields), u
        for f in want._fields:
            if f != "score":
                assert np.array_equal(g.field(f), want.field(f)), (u, f)


@pytest.mark.parametrize("toml", ["als-implicit.toml", "iknn-explicit.toml"])
def test_batched_paths_follow_a_retrain(gpu, ml_ds, toml):
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.training import TrainingOptions

    syn = _synthetic(ml_ds)
    pipe = Pipeline.load_config(GOLDEN / "pipelines" / toml)
    knn = toml.startswith("iknn")
    if not knn:
        pipe.node("scorer").component.config.epochs = 4
    lookup = pipe.node("history-lookup").component
    ml_users = [int(u) for u in ml_ds.users.ids()[::9]] + [-5]
    syn_users = [int(u) for u in syn.users.ids()[::6]] + [-5]

    pipe.train(ml_ds, TrainingOptions(rng=42))  # device state built from the first data
    _check_recommend(pipe, ml_users)
    if knn:
        _check_predict(pipe, ml_ds, ml_users[:40])
    pipe.train(syn, TrainingOptions(rng=43))  # every component retrained on the second
    _check_recommend(pipe, syn_users)
    if knn:
        _check_predict(pipe, syn, syn_users[:40])
    lookup.train(ml_ds)  # the lookup alone: the scorer keeps the second data's model
    _check_recommend(pipe, ml_users)
    if knn:
        _check_predict(pipe, ml_ds, ml_users[:40])
