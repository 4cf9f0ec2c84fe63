"""GPU: ``batch.predict`` for item-kNN pipelines as whole batches by user number
(``ItemKNNScorer.score_history_batch`` + csrc/predict_merge.hip) against the per-query
``rating-predictor`` composition it replaces -- score bits, ``nbr_counts``, ``is_fallback`` --
on ml-latest-small with ``iknn-explicit.toml`` and at the ML-25M shape."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"


def _per_query(pipe, pairs: dict) -> dict:
    """the per-query composition for every non-empty list (the per-query scorer cannot score an
    empty target list: lk_iknn_score_batch refuses the empty output buffers)"""
    from lkpy_amd.data import ItemList

    return {u: pipe.run("rating-predictor", query=u,
                        items=il if isinstance(il, ItemList) else ItemList(np.asarray(il)))
            for u, il in pairs.items() if len(il)}


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _assert_same(got, want: dict):
    "every list of ``got`` (an ItemListCollection) equals the per-query list, bit for bit"
    from lkpy_amd.data import ItemListCollection

    assert len(got) >= len(want)
    for k, g in got:  # the lists the per-query path cannot score are empty
        if k.user_id not in want:
            assert len(g) == 0 and g.field("score") is not None, k
    for u, w in want.items():
        g = got.lookup(u)
        assert g is not None, u
        assert np.array_equal(g.ids(), w.ids()), u
        assert list(g._fields) == list(w._fields), (u, list(g._fields), list(w._fields))
        assert np.array_equal(_bits(g.scores()), _bits(w.scores())), u
        for f in w._fields:
            if f != "score":
                assert np.array_equal(g.field(f), w.field(f)), (u, f)
    ref = ItemListCollection.from_dict(want, key=("user_id",)).to_df()
    df = got.to_df()
    assert sorted(df.columns) == sorted(ref.columns)
    pd.testing.assert_frame_equal(df, ref[df.columns], check_dtype=False)


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


@pytest.fixture(scope="module")
def iknn_pipe(gpu, ml_ds):
    from lkpy_amd.pipeline import Pipeline

    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "iknn-explicit.toml")
    pipe.train(ml_ds)
    return pipe


@pytest.fixture(scope="module")
def ml_pairs(ml_ds):
    "the golden pairs + an unknown user, unknown items, an empty list and a long random list"
    from lkpy_amd.data import ItemList

    known = pd.read_csv(GOLDEN / "item-item-preds.csv")
    pairs = {int(u): ItemList(g.item_id.values) for u, g in known.groupby("user_id", sort=False)}
    u0 = next(iter(pairs))
    pairs[u0] = ItemList(np.concatenate([pairs[u0].ids(), [-7, 10**9]]))  # unknown items
    pairs[999_999] = ItemList([1, 2, 3, 10**9])  # unknown user
    users = ml_ds.users.ids()
    rest = [int(u) for u in users if int(u) not in pairs]
    pairs[rest[0]] = ItemList(np.zeros(0, np.int64))  # empty target list
    rng = np.random.default_rng(5)
    for u in rest[1:40]:
        pairs[u] = ItemList(rng.choice(ml_ds.items.ids(), 60, replace=False))
    return pairs


def test_predict_equals_per_query_ml_small(iknn_pipe, ml_pairs):
    from lkpy_amd import batch

    want = _per_query(iknn_pipe, ml_pairs)
    got = batch.predict(iknn_pipe, ml_pairs)
    assert type(got._lists).__name__ == "_RaggedLists"  # the batched path
    _assert_same(got, want)
    fb = np.concatenate([il.field("is_fallback") for il in want.values()])
    assert fb.any() and not fb.all()
    assert got.lookup(999_999).field("nbr_counts") is None  # no history: no counts
    u_empty = next(u for u, il in ml_pairs.items() if len(il) == 0)
    assert len(got.lookup(u_empty)) == 0
    only = batch.predict(iknn_pipe, {u_empty: ml_pairs[u_empty]})  # nothing to score at all
    assert len(only) == 1 and len(only.lookup(u_empty)) == 0 and len(only.to_df()) == 0


@pytest.mark.parametrize("config", [{"damping": 5.0}, {"entities": ["item"]},
                                    {"damping": (3.0, 7.0), "entities": ["user"]}])
def test_predict_bias_variants_ml_small(iknn_pipe, ml_ds, ml_pairs, config):
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer
    from lkpy_amd.pipeline import predict_pipeline

    pipe = predict_pipeline(iknn_pipe.node("scorer").component)
    pipe.replace_component("fallback-predictor", BiasScorer, config)
    pipe.train(ml_ds)  # the lookup and the bias model (the scorer is trained)
    _assert_same(batch.predict(pipe, ml_pairs), _per_query(pipe, ml_pairs))


def test_predict_without_fallback_ml_small(iknn_pipe, ml_ds, ml_pairs):
    from lkpy_amd import batch
    from lkpy_amd.pipeline import predict_pipeline

    pipe = predict_pipeline(iknn_pipe.node("scorer").component, fallback=False)
    pipe.train(ml_ds)
    got = batch.predict(pipe, ml_pairs)
    _assert_same(got, _per_query(pipe, ml_pairs))
    assert "is_fallback" not in got.to_df().columns


def test_predict_dataframe_runs_no_per_query_component(iknn_pipe, ml_pairs, monkeypatch):
    """A test frame through ``batch.predict`` with the per-query components disabled: the whole
    batch goes by user number, nothing runs per query (and the lists are the per-query ones)."""
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer, FallbackScorer, UserTrainingHistoryLookup
    from lkpy_amd.data import ItemList, ItemListCollection

    rng = np.random.default_rng(11)
    rows = [(u, i) for u, il in ml_pairs.items() for i in il.ids()]
    df = pd.DataFrame(rows, columns=["user_id", "item_id"])
    df["rating"] = rng.uniform(0.5, 5.0, len(df)).astype(np.float32)
    df = df.sample(frac=1.0, random_state=3).reset_index(drop=True)  # users interleaved
    want = {}
    for u, g in df.groupby("user_id", sort=False):
        want[u] = iknn_pipe.run("rating-predictor", query=u,
                                items=ItemList(g.drop(columns="user_id")))

    def boom(*_a, **_k):
        raise AssertionError("per-query component called")

    monkeypatch.setattr(UserTrainingHistoryLookup, "__call__", boom)
    monkeypatch.setattr(BiasScorer, "__call__", boom)
    monkeypatch.setattr(FallbackScorer, "__call__", boom)
    got = batch.predict(iknn_pipe, df)
    assert [k.user_id for k in got.keys()] == list(pd.unique(df.user_id))
    _assert_same(got, want)
    # the reference's input form: a collection keyed by user_id
    ilc = ItemListCollection.from_dict(
        {u: ItemList(g.drop(columns="user_id")) for u, g in df.groupby("user_id", sort=False)},
        key=("user_id",))
    _assert_same(batch.predict(iknn_pipe, ilc), want)
    # several batches
    _assert_same(batch.predict(iknn_pipe, df, batch_size=7), want)


# ---- the ML-25M shape ------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ml25m(gpu):
    from lkpy_amd import synth
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.knn import ItemKNNScorer
    from lkpy_amd.pipeline import predict_pipeline

    ratings = synth.ml25m_like()
    n_u, n_i = ratings.shape
    ds = Dataset(Vocabulary(np.arange(n_u), "user", reorder=False),
                 Vocabulary(np.arange(n_i), "item", reorder=False),
                 np.repeat(np.arange(n_u, dtype=np.int32), np.diff(ratings.indptr)),
                 ratings.indices, {"rating": ratings.data})
    pipe = predict_pipeline(ItemKNNScorer(max_nbrs=100, min_nbrs=1, save_nbrs=100))
    pipe.train(ds)
    return ratings, ds, pipe


def _users(ratings, n, seed):
    rng = np.random.default_rng(seed)
    users = rng.choice(ratings.shape[0], n, replace=False)
    users[:3] = np.argsort(-np.diff(ratings.indptr))[:3]  # the three longest histories
    return users


def test_score_history_batch_matches_oracle_ml25m_shape(ml25m, oracle):
    import scipy.sparse as sps

    from lkpy_amd.matrix import csr_arrays

    ratings, ds, pipe = ml25m
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    users = _users(ratings, 2000, 44)
    n_i = ratings.shape[1]
    t_ptr = np.arange(len(users) + 1, dtype=np.int64) * 100
    t_idx = np.random.default_rng(45).integers(0, n_i, len(users) * 100).astype(np.int32)
    s, c = scorer.score_history_batch(lookup.batch(users), t_ptr, t_idx)
    s, c = s.cpu().numpy(), c.cpu().numpy()

    so, si, sv, shape = csr_arrays(scorer.sim_matrix)
    sims = sps.csr_array((np.asarray(sv), np.asarray(si), np.asarray(so)), shape=shape)
    r_ptr = np.zeros(len(users) + 1, np.int64)
    np.cumsum(np.diff(ratings.indptr)[users], out=r_ptr[1:])
    take = np.concatenate([np.arange(ratings.indptr[u], ratings.indptr[u + 1]) for u in users])
    r_idx = ratings.indices[take].astype(np.int32)
    r_val = (ratings.data[take].astype(np.float32) - scorer.item_means[r_idx]).astype(np.float32)
    ws, wc = oracle.iknn_score_batch(sims, r_ptr, r_idx, r_val, t_ptr, t_idx, 100, 1,
                                     oracle.num_threads())
    assert np.array_equal(c, wc)
    assert np.array_equal(np.isnan(s), np.isnan(ws))
    fin = ~np.isnan(ws)
    assert fin.sum() > 20_000  # (save_nbrs = 100: most random targets have no neighbour)
    assert np.array_equal(s[fin].view(np.uint32), ws[fin].astype(np.float32).view(np.uint32))


def test_predict_equals_per_query_ml25m_shape(ml25m):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    ratings, ds, pipe = ml25m
    users = _users(ratings, 1000, 46)
    rng = np.random.default_rng(47)
    items = rng.integers(0, ratings.shape[1] + 50, (len(users), 100))  # a few unknown items
    df = pd.DataFrame({"user_id": np.repeat(users, 100), "item_id": items.ravel()})
    got = batch.predict(pipe, df)
    want = {int(u): pipe.run("rating-predictor", query=int(u), items=ItemList(items[r]))
            for r, u in enumerate(users)}
    _assert_same(got, want)


def test_user_bias_of_long_rows_ml25m_shape(ml25m):
    """``lk_bias_user_offsets`` where NumPy's sum crosses its 8192-element blocks: the user bias of
    every user with a longer row against ``BiasModel.compute_for_items``."""
    from lkpy_amd.data import ItemList

    ratings, ds, pipe = ml25m
    lookup = pipe.node("history-lookup").component
    bias = pipe.node("fallback-predictor").component
    lens = np.diff(ratings.indptr)
    long_users = np.flatnonzero(lens > 8192)
    assert len(long_users) >= 1
    users = np.concatenate([long_users, _users(ratings, 200, 48)])
    ub, add = bias.user_offsets_batch(lookup.batch(users))
    ub, add = ub.cpu().numpy(), add.cpu().numpy()
    assert add.all()
    for r, u in enumerate(users):
        _, want = bias.model.compute_for_items(ItemList([0]), int(u), ds.user_row(int(u)))
        assert ub[r].view(np.uint32) == np.float32(want).view(np.uint32), (u, lens[u])
