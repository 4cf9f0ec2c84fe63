"""Host side of user-kNN's batched recommend path (no GPU): the per-user centres of provided
histories, the panel-row formula, and the attributes ``batch.recommend`` routes by."""
import numpy as np


def _dataset(rng, n_users=23, n_items=17):
    from lkpy_amd.data import Dataset

    users, items, ratings = [], [], []
    for u in range(n_users):
        m = int(rng.integers(1, n_items))
        its = rng.choice(n_items, m, replace=False)
        users += [100 + u] * m
        items += [int(i) + 1000 for i in its]
        ratings += list(rng.integers(1, 11, m) * 0.5)
    return Dataset.from_arrays(np.array(users), np.array(items),
                               np.array(ratings, dtype=np.float32))


def _trained_lookup(ds):
    from lkpy_amd.basic import UserTrainingHistoryLookup

    lookup = UserTrainingHistoryLookup()
    lookup.train(ds)
    return lookup


def test_history_centres_are_the_per_user_numpy_means(rng):
    from lkpy_amd.knn import UserKNNScorer

    ds = _dataset(rng)
    lookup = _trained_lookup(ds)
    scorer = UserKNNScorer(k=5)
    scorer.user_ratings = object()  # (only its identity is looked at: the cache key)
    got = scorer._history_centres(lookup)
    assert got.dtype == np.float32 and got.shape == (ds.user_count,)
    for num, uid in enumerate(ds.users.ids()):
        urv = np.require(lookup(int(uid)).query_items.field("rating"), dtype=np.float32)
        assert got[num].tobytes() == np.float32(float(urv.mean())).tobytes(), uid
    assert scorer._history_centres(lookup) is got  # cached per (lookup matrix, scorer)
    scorer.user_ratings = object()  # a retrain: computed again
    again = scorer._history_centres(lookup)
    assert again is not got and np.array_equal(again, got)


def test_panel_rows_formula():
    from lkpy_amd.data import Vocabulary
    from lkpy_amd.knn import UserKNNScorer

    scorer = UserKNNScorer()
    assert UserKNNScorer.PANEL_BYTES == 1 << 30
    for n_users, n_items, budget in [(671, 9125, 1 << 30), (671, 9125, 1 << 20), (7, 3, 1 << 30),
                                     (162541, 59047, 1 << 30), (10, 10, 1), (150, 90, 4 * 330 * 65)]:
        scorer.users = Vocabulary(np.arange(n_users), "user")
        scorer.items = Vocabulary(np.arange(n_items), "item")
        scorer.PANEL_BYTES = budget
        rows = scorer._panel_rows()
        assert rows >= 64 and rows % 64 == 0
        raw = budget // (4 * (2 * n_items + n_users))
        assert rows == max(64, raw // 64 * 64)


def test_batch_routes_user_knn_by_its_attributes(rng):
    from lkpy_amd import batch
    from lkpy_amd.knn import UserKNNScorer

    lookup = _trained_lookup(_dataset(rng))
    scorer = UserKNNScorer()
    assert scorer.accepts_history_batch is True
    assert callable(scorer.recommend_batch) and callable(scorer.dense_scores_batch)
    assert batch._takes_history_batches(scorer, lookup)
    assert batch._has_panels(scorer, lookup)
