"""The bias model on the device (csrc/bias.hip): the fit against ``BiasModel.learn`` on the host,
and the batch entry points over Bias pipelines against ``pipe.run`` per user.  Every comparison is
bit equality; the yardsticks (``learn(device=None)``, ``pipe.run``) are host code this change does
not touch."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bias_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_model(got, want):
    assert got.global_bias == want.global_bias
    assert R.same_bits(got.item_biases, want.item_biases)
    assert R.same_bits(got.user_biases, want.user_biases)
    assert (got.items is None) == (want.items is None)
    assert (got.users is None) == (want.users is None)


# ---- the fit ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_ds():
    return R.matrix_dataset()


def test_kernel_constants_are_the_test_matrix(gpu):
    "the matrix puts bins at the kernel's own seams: 64 | 65 and C - 1, C, C + 1, 3 C + 5"
    from lkpy_amd import _native

    lib = _native.load()
    assert lib.lk_bias_fit_short_max() == R.SHORT_MAX and lib.lk_bias_fit_chunk() == R.CHUNK


@pytest.mark.parametrize("entities", R.ENTITIES, ids="+".join)
def test_fit_is_the_hosts(gpu, fit_ds, entities):
    from lkpy_amd.basic import BiasModel

    for damping in R.DAMPINGS:
        want = BiasModel.learn(fit_ds, damping, entities=entities)
        got = BiasModel.learn(fit_ds, damping, entities=entities, device=gpu)
        assert want.device_biases is None and got.device_biases is not None
        _same_model(got, want)
        for dev, host in zip(got.device_biases, (got.item_biases, got.user_biases)):
            assert (dev is None) == (host is None)
            assert dev is None or np.array_equal(_bits(dev.cpu().numpy()), _bits(host))


def test_fit_repeats_and_takes_the_callers_matrices(gpu, fit_ds):
    from lkpy_amd import _device as D
    from lkpy_amd.basic import BiasModel

    ds = fit_ds
    first = BiasModel.learn(ds, 100 / 3, device=gpu)
    again = BiasModel.learn(ds, 100 / 3, device=gpu)
    _same_model(again, first)
    for wide in (False, True):  # (either offset width)
        ptr = ds._indptr.astype(np.int64 if wide else np.int32)
        csr = D.DeviceCSR.from_arrays(ptr, ds._cols, ds._attrs["rating"],
                                      (ds.user_count, ds.item_count), gpu)
        assert csr.is64 == wide
        csr_t = D.csr_transpose(csr, with_values=True)
        _same_model(BiasModel.learn(ds, 100 / 3, device=gpu, csr=csr, csr_t=csr_t), first)
        _same_model(BiasModel.learn(ds, 100 / 3, device=gpu, csr=csr), first)


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def test_trainers_fit_on_the_device(gpu, fit_ds, ml_ds):
    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.basic import BiasModel, BiasScorer
    from lkpy_amd.sklearn.svd import BiasedSVDScorer
    from lkpy_amd.training import TrainingOptions

    for ds in (fit_ds, ml_ds):
        for config in ({"damping": 100 / 3}, {"damping": (0.1, 5.0), "entities": ["item"]}):
            scorer = BiasScorer(**config)
            scorer.train(ds)
            _same_model(scorer.model, BiasModel.learn(ds, scorer.config.damping,
                                                      entities=scorer.config.entities))
            assert scorer.model.device_biases is not None
            assert scorer._device_item_biases() is scorer.model.device_biases[0]  # no re-upload
    svd = BiasedSVDScorer(embedding_size=8, damping=100 / 3)
    svd.train(ml_ds, TrainingOptions(rng=1))
    _same_model(svd.bias, BiasModel.learn(ml_ds, 100 / 3))
    mf = BiasedMFScorer(embedding_size=8, epochs=1, damping=(2.0, 100 / 3))
    mf.train(ml_ds, TrainingOptions(rng=1))
    _same_model(mf.bias, BiasModel.learn(ml_ds, (2.0, 100 / 3)))


# ---- scoring ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ml_run(ml_ds):
    "ml-latest-small plus one user without a training row; a trained std:topn-predict Bias pipeline"
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import Pipeline

    lonely = int(ml_ds.users.ids().max()) + 1
    users = Vocabulary(np.append(ml_ds.users.ids(), lonely), "user")
    ds = Dataset(users, ml_ds.items, ml_ds._rows, ml_ds._cols, dict(ml_ds._attrs))
    ds.item_attrs["protected"] = np.random.default_rng(20).random(ds.item_count) < 0.2
    pipe = Pipeline.load_config(GOLDEN / "pipelines" / "bias.toml")
    pipe.train(ds)
    uids = [int(u) for u in ml_ds.users.ids()[::9]] + [lonely, 10 ** 7]  # + empty row, unknown
    return ds, pipe, uids


def _same_lists(got, want, where=None):
    assert np.array_equal(got.ids(), want.ids()), where
    assert list(got._fields) == list(want._fields), where
    for f in want._fields:
        a, b = got.field(f), want.field(f)
        assert a.dtype == b.dtype, (where, f)
        if a.dtype == np.float32:
            assert np.array_equal(_bits(a), _bits(b)), (where, f)
        else:
            assert np.array_equal(a, b), (where, f)


def _targets(ds, uids, per_user, *, unknown_items=True, seed=3):
    "per user a list of item ids, some the user's own, some (``unknown_items``) in no vocabulary"
    rng = np.random.default_rng(seed)
    ids = ds.items.ids()
    out = {}
    for k, u in enumerate(uids):
        picks = rng.choice(ids, per_user, replace=False)
        if unknown_items and k % 3 == 0:
            picks[:: 4] = 10 ** 8 + np.arange(len(picks[::4]))
        out[u] = picks if k != 1 else picks[:0]  # (one empty list)
    return out


def _no_fallback(pipe):
    from lkpy_amd.pipeline import predict_pipeline

    bare = predict_pipeline(pipe.node("scorer").component, fallback=False)
    for name in ("history-lookup", "candidate-selector"):
        bare.nodes[name].component = pipe.nodes[name].component
    return bare


def test_batch_predict_and_score_are_the_pipeline_per_user(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    ds, pipe, uids = ml_run
    pairs = {u: ItemList(item_ids=t, rating=np.arange(len(t), dtype=np.float32))
             for u, t in _targets(ds, uids, 20).items()}
    bare = _no_fallback(pipe)
    assert batch._bias_predict_parts(pipe)[2] and not batch._bias_predict_parts(bare)[2]
    for p, fallback in ((pipe, True), (bare, False)):
        for size in (16384, 7):
            out = batch.predict(p, pairs, batch_size=size)
            assert len(out) == len(uids)
            for u in uids:
                one = p.run("rating-predictor", query=u, items=pairs[u])
                _same_lists(out.lookup(u), one, u)
                assert (out.lookup(u).field("is_fallback") is not None) == fallback
                assert not fallback or not out.lookup(u).field("is_fallback").any()
                assert not np.isnan(out.lookup(u).scores()).any()  # (unknown items too)
    scored = batch.score(pipe, pairs)
    for u in uids:
        _same_lists(scored.lookup(u), pipe.run("scorer", query=u, items=pairs[u]), u)
    # the user term is there for the known users, and only for them
    s_known = scored.lookup(uids[0]).scores()
    s_none = scored.lookup(uids[-1]).scores()
    nums = ds.items.numbers(pairs[uids[-1]].ids(), missing="negative")
    model = pipe.node("scorer").component.model
    base = np.full(len(nums), model.global_bias, np.float32)
    base[nums >= 0] += model.item_biases[nums[nums >= 0]]
    assert np.array_equal(_bits(s_none), _bits(base)) and len(s_known) == 20


def test_batch_recommend_is_the_pipeline_per_user(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasScorer
    from lkpy_amd.data import ItemList

    ds, pipe, uids = ml_run
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    assert batch._takes_history_batches(scorer, lookup)
    for n in (10, ds.item_count + 50, None):
        some = uids if n == 10 else uids[::8] + uids[-2:]
        out = batch.recommend(pipe, some, n)
        assert len(out) == len(some)
        for u in some:
            one = pipe.run("recommender", query=u, n=n)
            _same_lists(out.lookup(u), one, (n, u))
            row = ds.user_row(u)
            if row is not None and len(row):
                assert not np.isin(out.lookup(u).ids(), row.ids()).any()
        if n is None:
            assert len(out.lookup(some[-1])) == ds.item_count
    # more than one panel: 3 rows a panel
    want = batch.recommend(pipe, uids, 10)
    try:
        BiasScorer.PANEL_BYTES = 3 * 4 * ds.item_count
        assert scorer._panel_rows() == 3
        small = batch.recommend(pipe, uids, 10)
        idx, sc = scorer.recommend_batch(lookup.batch(uids), 10, exclude_history=False)
        on_dev = scorer.recommend_batch(lookup.batch(uids), 10, device_output=True)
    finally:
        BiasScorer.PANEL_BYTES = 1 << 30
    for u in uids:
        _same_lists(small.lookup(u), want.lookup(u), u)
    assert on_dev[0].is_cuda and on_dev[1].is_cuda
    # nothing excluded: the top of the whole catalogue, the user's own items among them
    own = 0
    for b, u in enumerate(uids):
        items = pipe.run("scorer", query=u, items=ItemList.from_vocabulary(ds.items)).top_n(10)
        assert np.array_equal(ds.items.ids(idx[b]), items.ids()), u
        assert np.array_equal(_bits(sc[b]), _bits(items.scores())), u
        row = ds.user_row(u)
        own += row is not None and bool(np.isin(items.ids(), row.ids()).any())
    assert own > 0


def test_candidate_lists_and_unknown_items(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList

    ds, pipe, uids = ml_run
    known = _targets(ds, uids, 40, unknown_items=False)
    out = batch.recommend(pipe, None, 10, candidates=known)
    every = batch.recommend(pipe, None, None, candidates=known, batch_size=5)
    for u in uids:
        _same_lists(out.lookup(u), pipe.run("recommender", query=u, items=ItemList(item_ids=known[u]), n=10),
                    u)
        _same_lists(every.lookup(u), pipe.run("recommender", query=u, items=ItemList(item_ids=known[u])), u)
    # an unknown item is scored, not NaN: pipe.run lists it under its id, and so does the batch call
    mixed = _targets(ds, uids, 40)
    out = batch.recommend(pipe, None, 10, candidates=mixed)
    listed = 0
    for u in uids:
        one = pipe.run("recommender", query=u, items=ItemList(item_ids=mixed[u]), n=10)
        _same_lists(out.lookup(u), one, u)
        listed += int((one.ids() >= 10 ** 8).sum())
    assert listed > 0


def test_stochastic_ranker_and_fair_reranker(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import Pipeline, topn_pipeline
    from lkpy_amd.reranking import FAIRReranker
    from lkpy_amd.stochastic import StochasticTopNRanker

    ds, pipe, uids = ml_run
    scorer = pipe.node("scorer").component
    some = uids[::6] + uids[-2:]

    def over(base):
        p = topn_pipeline(scorer)
        for name in ("history-lookup", "candidate-selector"):
            p.nodes[name].component = base.nodes[name].component
        return p

    drawn = over(pipe)
    drawn.replace_component("ranker", StochasticTopNRanker(rng=(7, "user")),
                            query="history-lookup")
    assert batch._has_panels(scorer, drawn.node("history-lookup").component)
    out = batch.recommend(drawn, some, 20)
    for u in some:
        _same_lists(out.lookup(u), drawn.run("recommender", query=u, n=20), u)
    fair = over(pipe)
    rr = FAIRReranker(n=20)
    rr.train(ds)
    fair.add_reranker(rr)
    out = batch.recommend(fair, some, 20)
    deep = batch.recommend(fair, some, 20, rerank_depth=200)
    moved = 0
    for u in some:
        _same_lists(out.lookup(u), fair.run("recommender", query=u, n=20), u)
        wide = pipe.run("recommender", query=u, n=200)
        _same_lists(deep.lookup(u), rr(items=wide, n=20), u)
        moved += not np.array_equal(deep.lookup(u).ids(), wide.ids()[:20])
    assert moved > 0
    # candidate lists under the reranker: by batches with the depth honoured; a list with an item
    # outside the vocabulary goes through pipe.run, which has no depth -- that is refused
    known = _targets(ds, some, 60, unknown_items=False)
    deep = batch.recommend(fair, None, 20, candidates=known, rerank_depth=50)
    for u in some:
        wide = pipe.run("recommender", query=u, items=ItemList(item_ids=known[u]), n=50)
        _same_lists(deep.lookup(u), rr(items=wide, n=20), u)
    mixed = _targets(ds, some, 60)
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(fair, None, 20, candidates=mixed, rerank_depth=50)
    out = batch.recommend(fair, None, 20, candidates=mixed)
    for u in some:
        _same_lists(out.lookup(u),
                    fair.run("recommender", query=u, items=ItemList(item_ids=mixed[u]), n=20), u)


def test_ties_after_the_user_term_go_to_the_lower_item(gpu):
    """Two base values one place apart that the user term merges: items 3 and 4 swap places
    between the two users, and runs of items with the same bias stay in item order."""
    from lkpy_amd import batch
    from lkpy_amd.basic import BiasModel, BiasScorer
    from lkpy_amd.data import Dataset, Vocabulary
    from lkpy_amd.pipeline import topn_pipeline

    ulp = np.float32(2.0 ** -22)  # a last place of a float32 in [2, 4)
    biases = np.array([0.25, 0.25, 0.25, 0.0, ulp, 0.25, -0.5, -0.5, 0.0, 0.0, 0.125, 0.125],
                      np.float32)
    # user 0 rates item 9 (bias 0) 4.5: ub = 1.5, and 3 + 1.5 = (3 + 2^-22) + 1.5 in float32;
    # user 1 rates it 3.25: ub = 0.25, which keeps the two apart
    ds = Dataset(Vocabulary(np.arange(3), "user", reorder=False),
                 Vocabulary(np.arange(len(biases)), "item", reorder=False),
                 np.array([0, 1], np.int32), np.array([9, 9], np.int32),
                 {"rating": np.array([4.5, 3.25], np.float32)})
    scorer = BiasScorer(damping=0.0)
    model = BiasModel(0.0, 3.0)
    model.items, model.item_biases = ds.items, biases
    model.users, model.user_biases = ds.users, np.zeros(3, np.float32)
    scorer.model = model
    pipe = topn_pipeline(scorer)
    for name in ("history-lookup", "candidate-selector"):  # (the scorer keeps the model above)
        pipe.node(name).component.train(ds)
    base = np.float32(3.0) + biases
    assert base[4] > base[3] and base[3] + np.float32(1.5) == base[4] + np.float32(1.5)
    assert base[3] + np.float32(0.25) != base[4] + np.float32(0.25)
    out = batch.recommend(pipe, [0, 1, 2], None)
    for u in (0, 1, 2):
        _same_lists(out.lookup(u), pipe.run("recommender", query=u), u)
    assert out.lookup(0).ids().tolist() == [0, 1, 2, 5, 10, 11, 3, 4, 8, 6, 7]
    assert out.lookup(1).ids().tolist() == [0, 1, 2, 5, 10, 11, 4, 3, 8, 6, 7]
    assert out.lookup(2).ids().tolist() == [0, 1, 2, 5, 10, 11, 4, 3, 8, 9, 6, 7]
    top = batch.recommend(pipe, [0, 1], 7)
    assert top.lookup(0).ids().tolist()[-1] == 3 and top.lookup(1).ids().tolist()[-1] == 4
