"""CPU: the host side of the batched ``BiasedMFScorer`` paths -- the NumPy restatement
(tests/als_explicit_batch_restatement.py) against the composition ``__call__`` runs
(``BiasModel.compute_for_items`` + ``finalize_scores``), which pipelines ``batch.predict`` takes by
user number, and what the scorer advertises."""
import numpy as np
import pytest

import als_explicit_batch_restatement as R


def _model(rng, n_items=40, n_users=9, damping=5.0):
    "a hand-made bias model and an untrained scorer around it (nothing here touches a device)"
    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.basic import BiasModel
    from lkpy_amd.data import Vocabulary

    items = Vocabulary(np.arange(100, 100 + n_items), "item")
    users = Vocabulary(np.arange(n_users), "user")
    bias = BiasModel(damping, float(rng.uniform(3.0, 4.0)))
    bias.items, bias.users = items, users
    bias.item_biases = rng.normal(0, 0.4, n_items).astype(np.float32)
    bias.user_biases = rng.normal(0, 0.3, n_users).astype(np.float32)
    scorer = BiasedMFScorer(embedding_size=4)
    scorer.items, scorer.users, scorer.bias = items, users, bias
    return scorer


def _history(rng, scorer, n, *, unknown=False, nan_rating=False):
    from lkpy_amd.data import ItemList

    ids = rng.choice(scorer.items.ids(), n, replace=False)
    ratings = rng.integers(1, 11, n).astype(np.float32) / 2
    if unknown and n:
        ids[n // 2] = 7  # not in the vocabulary
    if nan_rating and n:
        ratings[0] = np.nan
    return ItemList(item_ids=ids, rating=ratings)


@pytest.mark.parametrize("damping", [0.0, 5.0, (2.0, 3.0)])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 30])
@pytest.mark.parametrize("unknown", [False, True])
def test_fold_branch_restatement_equals_composition(damping, n, unknown):
    from lkpy_amd.basic import _damping
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(1000 * n + 7 * unknown)
    scorer = _model(rng, damping=damping)
    hist = _history(rng, scorer, n, unknown=unknown, nan_rating=(n == 9))
    bias = scorer.bias
    nums = hist.numbers(vocabulary=scorer.items, missing="negative")
    assert (nums < 0).any() == unknown
    # the fold-in's CSR row
    want_nums, want_res, u_off = scorer._residual_row(hist)
    biases, u_bias = bias.compute_for_items(hist, None, hist)
    got_nums, got_res, ub = R.residuals(hist.field("rating"), nums, bias.global_bias,
                                        bias.item_biases, _damping(damping, "user"))
    assert np.array_equal(got_nums, want_nums) and got_res.dtype == want_res.dtype == np.float32
    assert np.array_equal(R.bits(got_res), R.bits(want_res))
    assert np.float64(u_bias).tobytes() == np.float64(ub).tobytes() == np.float64(u_off).tobytes()
    # the final scores over targets with an unknown item
    tgt = ItemList(item_ids=np.concatenate([rng.choice(scorer.items.ids(), 25), [5]]))
    t_nums = tgt.numbers(vocabulary=scorer.items, missing="negative")
    dot = rng.normal(0, 0.5, len(tgt)).astype(np.float32)
    dot[t_nums < 0] = np.nan  # (item_scores leaves NaN under an unknown item)
    dot[0] = np.float32(1e-30)  # far below the biases' last bit: the double rounding case
    want = scorer.finalize_scores(None, ItemList(tgt, scores=dot), u_off).scores()
    got = R.finish(dot, t_nums, bias.global_bias, bias.item_biases, R.FOLD, ub)
    assert want.dtype == np.float32 and np.array_equal(R.bits(got), R.bits(want))
    assert np.isnan(got[-1]) and not np.isnan(got[:-1]).any()


def test_fold_branch_with_a_nan_user_bias():
    "every rating non-finite and no damping: 0 / 0 -> the bias is 0 and the scores stay float32"
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(3)
    scorer = _model(rng, damping=0.0)
    hist = ItemList(item_ids=scorer.items.ids()[:3],
                    rating=np.full(3, np.nan, dtype=np.float32))
    with np.errstate(invalid="ignore", divide="ignore"):
        want_nums, want_res, u_off = scorer._residual_row(hist)
    assert u_off == 0 and len(want_nums) == 0
    nums = hist.numbers(vocabulary=scorer.items, missing="negative")
    got_nums, got_res, ub = R.residuals(hist.field("rating"), nums, scorer.bias.global_bias,
                                        scorer.bias.item_biases, 0.0)
    assert ub == 0.0 and len(got_nums) == 0 and len(got_res) == 0
    tgt = ItemList.from_vocabulary(scorer.items)
    dot = rng.normal(0, 0.5, len(tgt)).astype(np.float32)
    dot[:4] = [0.0, -0.0, 1e-30, -1e-38]
    want = scorer.finalize_scores(None, ItemList(tgt, scores=dot), u_off).scores()
    got = R.finish(dot, np.arange(len(tgt)), scorer.bias.global_bias, scorer.bias.item_biases,
                   R.FOLD, ub)
    assert np.array_equal(R.bits(got), R.bits(want))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_stored_branch_restatement_equals_composition(seed):
    from lkpy_amd.data import ItemList

    rng = np.random.default_rng(seed)
    scorer = _model(rng)
    tgt = ItemList(item_ids=np.concatenate([scorer.items.ids(), [5]]))
    t_nums = tgt.numbers(vocabulary=scorer.items, missing="negative")
    dot = rng.normal(0, 0.5, len(tgt)).astype(np.float32)
    dot[t_nums < 0] = np.nan
    for user_num in (0, 4, 8):
        want = scorer.finalize_scores(user_num, ItemList(tgt, scores=dot), None).scores()
        got = R.finish(dot, t_nums, scorer.bias.global_bias, scorer.bias.item_biases, R.STORED,
                       scorer.bias.user_biases[user_num])
        assert np.array_equal(R.bits(got), R.bits(want))
    assert np.isnan(R.finish(dot, t_nums, scorer.bias.global_bias, scorer.bias.item_biases,
                             R.INVALID, 0.0)).all()


def test_scorer_advertises_the_batched_paths():
    from lkpy_amd.als import BiasedMFScorer

    assert BiasedMFScorer.accepts_history_batch is True
    assert BiasedMFScorer.returns_device_lists is True
    for name in ("recommend_batch", "dense_scores_batch", "score_batch", "predict_history_batch"):
        assert callable(getattr(BiasedMFScorer, name)), name
    assert BiasedMFScorer.PANEL_BYTES > 0


def test_fold_in_explicit_takes_pending():
    import inspect

    from lkpy_amd import _device as D

    sig = inspect.signature(D.fold_in_explicit)
    assert sig.parameters["pending"].default is None


# ---- which pipelines ``batch.predict`` runs by user number -----------------------------------


def _dataset(rng, n_users=12, n_items=30, f32=True):
    from lkpy_amd.data import Dataset, Vocabulary

    rows, cols = np.nonzero(rng.random((n_users, n_items)) < 0.3)
    ratings = rng.integers(1, 11, len(rows)) / 2
    return Dataset(Vocabulary(np.arange(n_users), "user"), Vocabulary(np.arange(n_items), "item"),
                   rows, cols, {"rating": ratings.astype(np.float32 if f32 else np.float64)})


def _trained_like(scorer, ds):
    "what ``BiasedMFTrainer`` leaves behind, without a device"
    from lkpy_amd.basic import BiasModel

    rng = np.random.default_rng(0)
    scorer.users, scorer.items = ds.users, ds.items
    scorer.bias = BiasModel.learn(ds, damping=5.0)
    scorer.item_embeddings = rng.normal(size=(len(ds.items), 4)).astype(np.float32)
    scorer.user_embeddings = rng.normal(size=(len(ds.users), 4)).astype(np.float32)
    return scorer


def _pipe(scorer, ds, *, fallback=True):
    from lkpy_amd.pipeline import predict_pipeline

    pipe = predict_pipeline(scorer, fallback=fallback)
    for name in ("history-lookup", "fallback-predictor"):
        node = pipe.nodes.get(name)
        if node is not None and node.component is not None:
            node.component.train(ds)
    return pipe


def test_batched_predict_parts_accepts_and_refuses():
    from lkpy_amd import batch
    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.basic import BiasScorer
    from lkpy_amd.data import Vocabulary

    rng = np.random.default_rng(5)
    ds = _dataset(rng)
    scorer = _trained_like(BiasedMFScorer(embedding_size=4), ds)
    # accepted: with the BiasScorer fallback, and without a merger
    parts = batch._batched_predict_parts(_pipe(scorer, ds))
    assert parts is not None and parts[0] is scorer and isinstance(parts[2], BiasScorer)
    parts = batch._batched_predict_parts(_pipe(scorer, ds, fallback=False))
    assert parts is not None and parts[2] is None
    # user_embeddings = False: no stored rows, no user vocabulary
    nouser = _trained_like(BiasedMFScorer(embedding_size=4, user_embeddings=False), ds)
    nouser.users = nouser.user_embeddings = None
    assert batch._batched_predict_parts(_pipe(nouser, ds)) is not None
    # refused: an untrained scorer
    assert batch._batched_predict_parts(_pipe(BiasedMFScorer(embedding_size=4), ds)) is None
    # refused: a bias model without the user (or the item) term
    for drop in ("user_biases", "item_biases"):
        part = _trained_like(BiasedMFScorer(embedding_size=4), ds)
        setattr(part.bias, drop, None)
        assert batch._batched_predict_parts(_pipe(part, ds)) is None, drop
    # refused: another item vocabulary, another user vocabulary
    other = _trained_like(BiasedMFScorer(embedding_size=4), ds)
    other.items = Vocabulary(np.arange(len(ds.items)) + 1, "item")
    assert batch._batched_predict_parts(_pipe(other, ds)) is None
    other = _trained_like(BiasedMFScorer(embedding_size=4), ds)
    other.users = Vocabulary(np.arange(len(ds.users)) + 1, "user")
    assert batch._batched_predict_parts(_pipe(other, ds)) is None
    # refused: a lookup without ratings; a fallback whose user term needs float32 ratings
    from lkpy_amd.data import Dataset

    bare = Dataset(ds.users, ds.items, ds._rows, ds._cols, {})
    pipe = _pipe(scorer, ds, fallback=False)
    pipe.node("history-lookup").component.train(bare)
    assert batch._batched_predict_parts(pipe) is None
    ds64 = _dataset(np.random.default_rng(5), f32=False)
    assert batch._batched_predict_parts(_pipe(_trained_like(BiasedMFScorer(embedding_size=4),
                                                            ds64), ds64)) is None
    # refused: a merger that is no FallbackScorer over a trained BiasScorer
    pipe = _pipe(scorer, ds)
    pipe.node("fallback-predictor").component = BiasScorer()
    assert batch._batched_predict_parts(pipe) is None
    # refused: a lookup without ``batch``
    pipe = _pipe(scorer, ds)

    class _Plain:
        interactions = pipe.node("history-lookup").component.interactions

    pipe.node("history-lookup").component = _Plain()
    assert batch._batched_predict_parts(pipe) is None


def test_lookup_retrain_drops_its_device_cache():
    "the HBM copy of the training matrix (and ``ratings_finite``) must not outlive a retrain"
    from lkpy_amd.basic import UserTrainingHistoryLookup

    lookup = UserTrainingHistoryLookup()
    lookup.train(_dataset(np.random.default_rng(1)))
    lookup.__dict__["_dev"] = {"matrix": ((lookup.interactions,), {"stale": True})}
    lookup.train(_dataset(np.random.default_rng(2)))
    assert "_dev" not in lookup.__dict__
