"""FA*IR off the device: the configuration, the thresholds and the adjusted significance against
the paper and the reference's recorded values, how the protected flag is read, the trained state,
and the reranker slot of the pipeline."""

from __future__ import annotations

import json
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fair_restatement as R  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "fair_thresholds.json").read_text())


def _dataset(flags=None, n_items=12, name="protected"):
    from lkpy_amd.data import Dataset

    users = np.repeat(np.arange(4), 3)
    items = np.arange(12) % n_items
    ds = Dataset.from_arrays(users, items, all_item_ids=np.arange(n_items))
    if flags is not None:
        ds.item_attrs[name] = flags
    return ds


def test_config_validation():
    from pydantic import ValidationError

    from lkpy_amd import _native
    from lkpy_amd.reranking import FAIRReranker, FAIRRerankerConfig

    cfg = FAIRRerankerConfig(n=10)
    assert (cfg.p, cfg.alpha, cfg.protected_attribute) == (0.5, 0.1, "protected")
    for bad in ({"n": 0}, {"n": -3}, {}, {"n": 10, "p": 0.0}, {"n": 10, "p": 1.0},
                {"n": 10, "p": -0.1}, {"n": 10, "alpha": 0.0}, {"n": 10, "alpha": 1.0},
                {"n": 10, "alpha": 1.5}, {"n": 10, "depth": 3}):
        with pytest.raises(ValidationError):
            FAIRRerankerConfig(**bad)
    assert _native.FAIR_MAX_N >= 1024
    FAIRRerankerConfig(n=_native.FAIR_MAX_N)
    with pytest.raises(ValueError, match=str(_native.FAIR_MAX_N)):
        FAIRRerankerConfig(n=_native.FAIR_MAX_N + 1)
    with pytest.raises(ValueError, match=str(_native.FAIR_MAX_N)):
        FAIRReranker(n=_native.FAIR_MAX_N + 1)
    assert FAIRReranker({"n": 7, "p": 0.3}).config.p == 0.3
    # the library was built with the limit the validator uses
    assert _native.load(build_if_missing=True).lk_fair_max_n() == _native.FAIR_MAX_N


def test_library_validates_before_any_device_work():
    import ctypes

    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    one = ctypes.c_void_p(64)  # (never dereferenced: validation comes first)
    null = ctypes.c_void_p(0)
    args = lambda **k: [k.get("lists", one), 2, 8, 8, null, null, k.get("flags", one), 5,  # noqa: E731
                        k.get("m", one), k.get("n_table", 10), k.get("n_out", 10),
                        k.get("out", one), null, null, null]
    assert lib.lk_fair_rerank(*args(out=null)) == _native.LK_E_INVALID
    assert b"null" in lib.lk_last_error()
    assert lib.lk_fair_rerank(*args(lists=null)) == _native.LK_E_INVALID
    assert lib.lk_fair_rerank(*args(flags=null)) == _native.LK_E_INVALID
    assert lib.lk_fair_rerank(*args(m=null)) == _native.LK_E_INVALID
    assert lib.lk_fair_rerank(*args(n_out=11)) == _native.LK_E_INVALID
    assert b"n_out" in lib.lk_last_error()
    big = _native.FAIR_MAX_N + 1
    assert lib.lk_fair_rerank(*args(n_table=big, n_out=big)) == _native.LK_E_INVALID
    assert str(_native.FAIR_MAX_N).encode() in lib.lk_last_error()


def test_thresholds_of_the_paper():
    from lkpy_amd import reranking as K

    m = K.m_table(10, 0.5, 0.1)  # Table 2 of the paper, raw alpha = 0.1
    assert m[3] == 1 and m[6] == 2 and m[8] == 3
    assert list(m) == list(R.thresholds(10, 0.5, 0.1))
    assert list(K.block_sizes([0, 0, 0, 1, 1, 1, 2, 2, 3])) == [4, 3, 2]
    assert R.blocks([0, 0, 0, 1, 1, 1, 2, 2, 3]) == [4, 3, 2]
    assert list(K.block_sizes([0, 0, 0])) == [] and R.blocks([0, 0]) == []
    assert abs(K.adjusted_alpha(10, 0.5, 0.1) - 0.0625) < 1e-9
    assert list(K.m_table(10, 0.5, K.adjusted_alpha(10, 0.5, 0.1))) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    a100 = K.adjusted_alpha(100, 0.5, 0.1)
    assert abs(a100 - 0.0204798) < 1e-6 and K.m_table(100, 0.5, a100)[-1] == 40


def test_train_reproduces_the_reference(golden):
    from lkpy_amd.reranking import FAIRReranker

    assert len(golden["grid"]) == 63
    ds = _dataset(np.zeros(12, dtype=bool))
    for g in golden["grid"]:
        rr = FAIRReranker(n=g["n"], p=g["p"], alpha=g["alpha"])
        rr.train(ds)
        assert abs(rr.alpha_c - g["alpha_c"]) <= 1e-12, g
        assert [int(x) for x in rr.m_list] == g["m_list"], (g["n"], g["p"], g["alpha"])
        if g["n"] <= 100:  # (the restatement agrees too; n = 1000 left to the component)
            assert abs(R.adjusted_alpha(g["n"], g["p"], g["alpha"]) - g["alpha_c"]) <= 1e-12
            assert list(R.thresholds(g["n"], g["p"], g["alpha_c"])) == g["m_list"]


def test_restatement_loop_is_the_reference_loop(golden):
    "the reference's own __call__ on the recorded lists == the restatement's greedy loop"
    lists = R.golden_lists()
    assert set(lists) == set(golden["lists"])
    m_of = {(g["n"], g["p"], g["alpha"]): g["m_list"] for g in golden["grid"]}
    moved = 0
    for name, (flags, n, p, alpha, ask) in lists.items():
        rec = golden["lists"][name]
        assert rec["flags"] == [int(f) for f in flags]
        t = R.rerank_flags(flags, m_of[(n, p, alpha)], ask or n)
        assert list(t.positions) == rec["positions"], name
        moved += list(t.positions) != list(range(len(t.positions)))
    assert moved >= 5
    assert golden["lists"]["paper-example"]["positions"] == [0, 1, 2, 6, 3, 4, 8, 5, 7, 9]


def test_flag_reading_rule_and_missing_attribute():
    from lkpy_amd.reranking import FAIRReranker

    vals = [1, True, 2, float("nan"), None, 0, False, 1.0, "yes", np.True_, np.int64(1), -1]
    rr = FAIRReranker(n=4)
    rr.train(_dataset(vals))
    assert rr.protected_attributes.dtype == np.bool_
    assert list(rr.protected_attributes) == [True, True, False, False, False, False, False, True,
                                             False, True, True, False]
    import pandas as pd

    rr.train(_dataset(pd.Series([True, False] * 6)))
    assert list(rr.protected_attributes) == [True, False] * 6
    rr.train(_dataset(np.arange(12) % 3))
    assert list(rr.protected_attributes) == [x == 1 for x in np.arange(12) % 3]

    other = FAIRReranker(n=4, protected_attribute="minority")
    with pytest.raises(ValueError) as e:
        other.train(_dataset(np.zeros(12)))
    assert str(e.value) == "Dataset is missing required 'minority' attribute for item entities"
    assert not other.is_trained()
    other.train(_dataset(np.ones(12), name="minority"))
    assert other.is_trained() and other.protected_attributes.all()
    with pytest.raises(ValueError):
        FAIRReranker(n=4).train(_dataset(np.zeros(5)))  # not one value per item


def test_trained_state_and_pickle():
    from lkpy_amd.pipeline import Component
    from lkpy_amd.reranking import FAIRReranker
    from lkpy_amd.training import Trainable

    rr = FAIRReranker(n=10)
    assert isinstance(rr, Component) and isinstance(rr, Trainable) and not rr.is_trained()
    ds = _dataset(np.arange(12) % 2 == 0)
    rr.train(ds)
    assert rr.is_trained() and rr.vocab is ds.items
    assert abs(rr.alpha_c - 0.0625) < 1e-9 and list(rr.m_list) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    rr.__dict__["_dev"] = {"fair": ((), object())}  # a device copy is never pickled
    back = pickle.loads(pickle.dumps({"rr": rr}))["rr"]
    assert "_dev" not in back.__dict__ and back.is_trained()
    assert back.alpha_c == rr.alpha_c and np.array_equal(back.m_list, rr.m_list)
    assert np.array_equal(back.protected_attributes, rr.protected_attributes)
    assert back.vocab == rr.vocab and back.config == rr.config
    # requested lengths: above the configured n is an error, below it a warning
    with pytest.raises(ValueError, match="exceeds configured"):
        rr._length(11)
    assert rr._length(None) == 10 and rr._length(10) == 10 and rr._length(4) == 4


def test_splits_carry_the_flag():
    "a reranker trains on the training half of a split: the flag comes along"
    from lkpy_amd import splitting
    from lkpy_amd.reranking import FAIRReranker

    flags = np.arange(12) % 2 == 0
    split = splitting.sample_users(_dataset(flags), 2, splitting.SampleN(1), rng=5)
    assert split.train.item_attrs["protected"] is flags
    rr = FAIRReranker(n=3)
    rr.train(split.train)
    assert np.array_equal(rr.protected_attributes, flags)


def _shape(pipe):
    "what two pipelines must share to be the same pipeline"
    return ({k: (type(n.component).__name__, n.kind, dict(n.wiring),
                 None if n.component is None else n.component.dump_config())
             for k, n in pipe.nodes.items()}, dict(pipe.aliases), pipe.default)


def test_pipeline_reranker_slot():
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.pipeline import Pipeline, predict_pipeline, topn_pipeline
    from lkpy_amd.reranking import FAIRReranker

    plain = topn_pipeline(ImplicitMFScorer(embedding_size=8), n=20)
    assert plain.aliases["recommender"] == "ranker" and plain.default == "recommender"
    assert "reranker" not in plain.nodes
    # without a reranker: the pipelines of before, keyword or not
    assert _shape(topn_pipeline(ImplicitMFScorer(embedding_size=8), n=20, reranker=None)) == \
        _shape(plain)
    assert _shape(predict_pipeline(ImplicitMFScorer(embedding_size=8), reranker=None)) == \
        _shape(predict_pipeline(ImplicitMFScorer(embedding_size=8)))
    base = Pipeline.std_topn(None, {"default_length": 20})
    base.replace_component("scorer", ImplicitMFScorer(embedding_size=8))
    assert _shape(base) == _shape(plain)

    for make in (lambda rr: topn_pipeline(ImplicitMFScorer(embedding_size=8), n=20, reranker=rr),
                 lambda rr: predict_pipeline(ImplicitMFScorer(embedding_size=8), n=20,
                                             reranker=rr)):
        rr = FAIRReranker(n=20)
        pipe = make(rr)
        node = pipe.nodes["reranker"]
        assert node.component is rr and node.wiring == {"items": "ranker", "n": "n"}
        assert pipe.aliases["recommender"] == "reranker" and pipe.default == "recommender"
        assert pipe.node("recommender") is node and pipe.node("ranker").component is not rr
    # add_reranker by class + config, as add_component takes them
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=8))
    assert pipe.add_reranker(FAIRReranker, {"n": 5, "p": 0.25}) == "reranker"
    assert pipe.node("recommender").component.config.p == 0.25
    without = {k: v for k, v in _shape(pipe)[0].items() if k != "reranker"}
    assert without == _shape(topn_pipeline(ImplicitMFScorer(embedding_size=8)))[0]

    cfg = {"options": {"base": "std:topn"},
           "components": {"scorer": {"class": "lkpy_amd.als.ImplicitMFScorer",
                                     "config": {"embedding_size": 8}},
                          "reranker": {"class": "lkpy_amd.reranking.FAIRReranker",
                                       "config": {"n": 10, "alpha": 0.2}}}}
    pipe = Pipeline.from_config(cfg)
    node = pipe.nodes["reranker"]
    assert isinstance(node.component, FAIRReranker) and node.component.config.alpha == 0.2
    # the reference's own class path names the mirror where LensKit itself is not importable
    from lkpy_amd.pipeline import import_path_string

    named = import_path_string("lenskit.reranking.FAIRReranker")
    assert named is FAIRReranker or named.__module__.startswith("lenskit.")
    assert node.wiring == {"items": "ranker", "n": "n"}
    assert pipe.aliases["recommender"] == "reranker" and pipe.default == "recommender"
    # explicit inputs: the component is wired as the file says and the alias stays
    cfg["components"]["reranker"]["inputs"] = {"items": "scorer"}
    pipe = Pipeline.from_config(cfg)
    assert pipe.nodes["reranker"].wiring == {"items": "scorer"}
    assert pipe.aliases["recommender"] == "ranker"
    del cfg["components"]["reranker"]
    assert _shape(Pipeline.from_config(cfg))[1] == {"recommender": "ranker"}


def test_pipeline_runs_a_reranker_and_trains_it():
    "the slot on the host, with a reranker that needs no device: run, train order, batch fallback"
    from lkpy_amd import batch
    from lkpy_amd.data import ItemList
    from lkpy_amd.pipeline import Component, topn_pipeline
    from lkpy_amd.reranking import FAIRReranker

    class Scores(Component):
        items = None

        def __call__(self, query, items):
            return ItemList(items, scores=-np.asarray(items.ids(), dtype=np.float32))

    class Top(Component):  # (the package's ranker selects on the device)
        def __call__(self, items, n=None):
            order = np.argsort(-items.scores(), kind="stable")[:n]
            return ItemList(items[order], ordered=True)

    class Reverse(Component):
        seen = None

        def is_trained(self):
            return self.seen is not None

        def train(self, data, options=None):
            self.seen = data

        def __call__(self, items, n=None):
            return ItemList(items[np.arange(len(items))[::-1]], ordered=True)

    ds = _dataset()
    pipe = topn_pipeline(Scores(), reranker=Reverse())
    pipe.replace_component("ranker", Top())
    pipe.train(ds)
    assert pipe.nodes["reranker"].component.seen is ds
    user = ds.users.id(0)
    ranked = pipe.run("ranker", query=user, n=3)
    got = pipe.run(query=user, n=3)
    assert len(got) == 3 and got.ordered and list(got.ids()) == list(ranked.ids())[::-1]
    assert np.array_equal(got.scores(), ranked.scores()[::-1])
    # a reranker without rerank_batch: batch.recommend runs the pipeline per user
    out = batch.recommend(pipe, [user], 3)
    assert list(out.lookup(user).ids()) == list(got.ids())
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(pipe, [user], 3, rerank_depth=6)
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(topn_pipeline(Scores()), [user], 3, rerank_depth=6)
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(topn_pipeline(Scores(), reranker=FAIRReranker(n=3)), [user], 3,
                        rerank_depth=2)  # below n


def test_reranking_needs_the_device():
    "no host path: without a GPU the reranker raises instead of looping in Python"
    import torch

    from lkpy_amd import _native
    from lkpy_amd.data import ItemList
    from lkpy_amd.reranking import FAIRReranker

    if torch.cuda.is_available():
        return
    rr = FAIRReranker(n=4)
    rr.train(_dataset(np.arange(12) % 2 == 0))
    with pytest.raises(_native.BackendUnavailable):
        rr(ItemList(np.arange(6)))
    with pytest.raises(_native.BackendUnavailable):
        rr.rerank_batch(np.zeros((2, 6), np.int32))
