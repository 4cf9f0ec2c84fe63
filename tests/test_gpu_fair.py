"""FA*IR on the device against the restatement (tests/fair_restatement.py): lists, positions and
score bits are compared exactly.  Shapes are the smallest at which the kernel takes another path:
rows around its 64-entry chunks, output lengths around 64, the LDS limit, batches that do not fill
the last workgroup."""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fair_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
N_ITEMS = 1000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_TRAINED = {}


def _reranker(table, n=100, p=0.5, alpha=0.1):
    "a trained reranker over items 0..len(table)-1 with the given flags (thresholds cached)"
    from lkpy_amd.data import Dataset
    from lkpy_amd.reranking import FAIRReranker

    table = np.asarray(table)
    ds = Dataset.from_arrays([0, 0], [0, len(table) - 1], all_item_ids=np.arange(len(table)))
    ds.item_attrs["protected"] = table
    rr = FAIRReranker(n=n, p=p, alpha=alpha)
    if (n, p, alpha) in _TRAINED:
        rr.alpha_c, m = _TRAINED[(n, p, alpha)]
        rr.m_list = m.copy()
        rr.protected_attributes = np.equal(table, True)
        rr.vocab = ds.items
    else:
        rr.train(ds)
        _TRAINED[(n, p, alpha)] = (rr.alpha_c, rr.m_list.copy())
    return rr


def _score_bits(shape, seed):
    "arbitrary float32 bit patterns (NaNs and infinities among them): scores are only carried"
    return np.random.default_rng(seed).integers(0, 2**32, size=shape, dtype=np.uint32) \
        .view(np.float32)


def _check_properties(lists, table, m, out_pos, out_items, traces, lengths=None):
    "what holds for any FA*IR output (checked on the DEVICE's arrays)"
    for r, t in enumerate(traces):
        ln = R.row_length(lists[r], None if lengths is None else lengths[r])
        k = min(out_pos.shape[1], ln)
        pos = out_pos[r, :k]
        assert (out_pos[r, k:] == -1).all() and (out_items[r, k:] == -1).all()
        assert ((pos >= 0) & (pos < ln)).all() and len(set(pos.tolist())) == k  # a sub-permutation
        assert np.array_equal(out_items[r, :k], lists[r, pos])
        if t.constrained:
            got = np.cumsum(R.item_flags(out_items[r, :k], table))
            assert (got >= np.asarray(m[:k])).all(), r


def _compare(rr, lists, n, *, lengths=None, scores=None, check=True):
    """``rerank_batch`` and ``lk_fair_rerank``'s positions against the restatement, exactly; host
    arrays and device tensors in; returns the restatement's traces"""
    import torch

    from lkpy_amd import _device as D

    lists = np.ascontiguousarray(lists, dtype=np.int32)
    table, m = rr.protected_attributes, rr.m_list
    w_items, w_scores, w_pos, traces = R.rerank_rows(lists, table, m, n, lengths=lengths,
                                                     scores=scores)
    g_items, g_scores = rr.rerank_batch(lists, scores, n, lengths=lengths)
    assert g_items.dtype == np.int32 and g_items.shape == (len(lists), n)
    assert np.array_equal(g_items, w_items)
    if scores is None:
        assert g_scores is None
    else:
        assert np.array_equal(_bits(g_scores), _bits(w_scores))
    # device tensors in, device tensors out: the same bits
    dev = D.device()
    d_lists = torch.from_numpy(lists).to(dev)
    d_scores = None if scores is None else torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    d_len = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(dev)
    d_items, d_sc = rr.rerank_batch(d_lists, d_scores, n, lengths=d_len, device_output=True)
    assert d_items.is_cuda and np.array_equal(d_items.cpu().numpy(), w_items)
    if scores is not None:
        assert d_sc.is_cuda and np.array_equal(_bits(d_sc.cpu().numpy()), _bits(w_scores))
    flags, d_m = rr._device_tables()
    _i, _s, d_pos = D.fair_rerank(d_lists, flags, d_m, n, lengths=d_len, want_pos=True)
    g_pos = d_pos.cpu().numpy()
    assert np.array_equal(g_pos, w_pos)
    if check:
        _check_properties(lists, table, m, g_pos, g_items, traces, lengths)
    return traces, w_items, w_scores


# ---- the recorded example ------------------------------------------------------------------------

def test_fixed_example(gpu):
    from lkpy_amd.data import Dataset, ItemList
    from lkpy_amd.reranking import FAIRReranker

    known = np.array([1, 2, 3, 4, 5, 31, 32, 33, 34])  # 35 is unknown to the dataset
    ds = Dataset.from_arrays([7, 7], [1, 2], all_item_ids=known)
    ds.item_attrs["protected"] = np.isin(known, [32, 34])
    rr = FAIRReranker(n=10, p=0.5, alpha=0.1)
    rr.train(ds)
    ids = np.array([1, 2, 3, 4, 5, 31, 32, 33, 34, 35])
    want = [1, 2, 3, 32, 4, 5, 34, 31, 33, 35]
    want_pos = [int(np.flatnonzero(ids == i)[0]) for i in want]
    scores = np.linspace(5, 1, 10).astype(np.float32)
    tag = np.arange(10) * 10
    out = rr(ItemList(ids, scores=scores, tag=tag, ordered=True))
    assert out.ordered and list(out.ids()) == want
    assert np.array_equal(_bits(out.scores()), _bits(scores[want_pos]))
    assert list(out.field("tag")) == [p * 10 for p in want_pos]
    assert list(rr(ItemList(ids), n=10).ids()) == want
    assert list(rr(ItemList(ids), n=4).ids()) == want[:4]  # (n below the configured n: warned)
    assert list(rr(ItemList(ids[:3])).ids()) == [1, 2, 3] and len(rr(ItemList(ids[:0]))) == 0
    with pytest.raises(ValueError, match="exceeds configured"):
        rr(ItemList(ids), n=11)
    # the same through rerank_batch with lengths: 35 is a negative number inside the row
    nums = ds.items.numbers(ids, missing="negative")
    assert nums[-1] == -1
    row = np.full((1, 16), -1, np.int32)
    row[0, :10] = nums
    sc = np.full((1, 16), np.nan, np.float32)
    sc[0, :10] = scores
    items, got_sc = rr.rerank_batch(row, sc, lengths=np.array([10], np.int32))
    assert items.shape == (1, 10) and list(items[0]) == list(nums[want_pos])
    assert np.array_equal(_bits(got_sc[0]), _bits(scores[want_pos]))
    # without lengths the row ends at its first negative entry: 35 is padding then
    items, _ = rr.rerank_batch(row)
    assert list(items[0]) == list(nums[want_pos[:-1]]) + [-1]


def test_recorded_reference_lists(gpu):
    "the reference's own __call__ output (tests/golden/fair_thresholds.json) from the kernel"
    golden = json.loads((GOLDEN / "fair_thresholds.json").read_text())
    for name, (flags, n, p, alpha, ask) in R.golden_lists().items():
        rr = _reranker(flags, n, p, alpha)
        row = np.arange(len(flags), dtype=np.int32).reshape(1, -1)
        items, _ = rr.rerank_batch(row, n=ask, lengths=np.array([len(flags)], np.int32))
        want = golden["lists"][name]["positions"]
        assert list(items[0][:len(want)]) == want and (items[0][len(want):] == -1).all(), name


# ---- chunk edges -----------------------------------------------------------------------------------

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)


def _pattern(name):
    pos = np.arange(N_ITEMS)
    if name == "none":
        return np.zeros(N_ITEMS, bool)
    if name == "all":
        return np.ones(N_ITEMS, bool)
    if name == "from64":
        return pos >= 64
    if name == "from128":
        return pos >= 128
    if name == "last":
        return np.zeros(N_ITEMS, bool)  # (set per row below: the row's last position)
    share = float(name)
    return np.random.default_rng(int(share * 100)).random(N_ITEMS) < share


def _edge_batch(name):
    """rows of every length in LENGTHS under one stride, twice: item number = position, and a
    permutation of the items (the flags then sit elsewhere in every row)"""
    rng = np.random.default_rng(11)
    table = _pattern(name)
    rows, lengths = [], []
    for k, ln in enumerate(LENGTHS):
        for perm in (False, True):
            row = np.full(N_ITEMS, -1, np.int32)
            row[:ln] = rng.permutation(N_ITEMS)[:ln] if perm and name != "last" else np.arange(ln)
            rows.append(row)
            lengths.append(ln)
    lists = np.stack(rows)
    if name == "last":  # a single protected item, at each row's last position
        lists = lists.copy()
        for r, ln in enumerate(lengths):
            if ln:
                lists[r, ln - 1] = N_ITEMS - 1
        table[N_ITEMS - 1] = True
    return table, lists, np.asarray(lengths, np.int32)


@pytest.mark.parametrize("name", ["none", "all", "from64", "from128", "last", "0.05", "0.2", "0.5"])
def test_chunk_edges(gpu, name):
    table, lists, lengths = _edge_batch(name)
    rr = _reranker(table, 100)
    scores = _score_bits(lists.shape, 5)
    for n in (1, 63, 64, 65, 100):  # n_out > L, < L, = config.n, < config.n
        traces, _, _ = _compare(rr, lists, n, lengths=lengths, scores=scores)
        # trailing -1 padding: no lengths needed, the same lists
        a, b = rr.rerank_batch(lists, scores, n)
        c, d = rr.rerank_batch(lists, scores, n, lengths=lengths)
        assert np.array_equal(a, c) and np.array_equal(_bits(b), _bits(d))
        if name == "all":
            assert all(t.u_dry for t, ln in zip(traces, lengths) if ln)
        if name in ("from64", "from128") and n == 100:
            # promotions cross chunks: a protected item from beyond the first chunk(s) moved up
            first = 64 if name == "from64" else 128
            long = [t for t, ln in zip(traces[::2], lengths[::2]) if ln > first]  # (items in order)
            assert long and all((t.positions[:first] >= first).any() for t in long)
    with pytest.raises(ValueError, match="exceeds configured"):
        rr.rerank_batch(lists, scores, 101)


def test_negative_entries_inside_a_length(gpu):
    "with lengths a negative entry is an unknown item: unprotected, kept; so is a number >= n_items"
    table = np.random.default_rng(3).random(N_ITEMS) < 0.3
    rng = np.random.default_rng(4)
    lists = rng.integers(0, N_ITEMS, size=(6, 150)).astype(np.int32)
    lists[rng.random(lists.shape) < 0.1] = -1
    lists[rng.random(lists.shape) < 0.05] = N_ITEMS + 7
    lengths = np.array([150, 149, 100, 64, 1, 0], np.int32)
    rr = _reranker(table, 100)
    _t, w_items, _s = _compare(rr, lists, 100, lengths=lengths,
                               scores=_score_bits(lists.shape, 6),
                               check=False)  # (repeated item numbers: positions are compared)
    assert (w_items[0] == -1).any() and (w_items[0] == N_ITEMS + 7).any()


# ---- power: the inputs make the loop do something ---------------------------------------------------

def test_power_conditions_and_random_rows(gpu):
    n, L, B = 100, 400, 300
    for share in (0.2, 0.05, 0.5):
        rng = np.random.default_rng(int(share * 1000))
        table = rng.random(4 * N_ITEMS) < share
        lists = np.stack([rng.permutation(4 * N_ITEMS)[:L] for _ in range(B)]).astype(np.int32)
        rr = _reranker(table, n)
        _items, _sc, w_pos, traces = R.rerank_rows(lists, table, rr.m_list, n)
        moved = sum(not np.array_equal(t.positions, np.arange(n)) for t in traces)
        if share == 0.2:  # room to promote from: the lists move, the constraints are met
            assert moved >= B // 2 and sum(t.constrained for t in traces) >= B // 2
        if share == 0.05:
            assert any(t.p_dry_short for t in traces)
        if share == 0.5:
            assert moved < B  # at least one row already fair
        _compare(rr, lists, n, scores=_score_bits(lists.shape, 9))
        if share == 0.05:  # at L = n nothing can be promoted into the list: P runs dry
            short = lists[:, :n]
            assert all(t.p_dry_short for t in R.rerank_rows(short, table, rr.m_list, n)[3])
            _compare(rr, short, n)
    # every item protected: U is empty from the first slot on
    table = np.ones(N_ITEMS, bool)
    lists = np.stack([np.random.default_rng(r).permutation(N_ITEMS)[:130] for r in range(5)])
    traces, _, _ = _compare(_reranker(table, n), lists.astype(np.int32), n)
    assert all(t.u_dry for t in traces)


# ---- threshold extremes -----------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [1e-10, 0.3])
def test_p09_thresholds(gpu, alpha):
    rng = np.random.default_rng(17)
    n = 64
    for share in (0.3, 0.9):
        table = rng.random(N_ITEMS) < share
        rr = _reranker(table, n, 0.9, alpha)
        if alpha == 0.3:  # promotions forced at most positions
            assert (np.diff(rr.m_list, prepend=0) > 0).sum() > n // 2
        else:  # nothing asked of the first slots
            assert rr.m_list[0] == 0 and 1 <= rr.m_list[-1] < n
        lists = np.stack([rng.permutation(N_ITEMS)[:300] for _ in range(9)]).astype(np.int32)
        traces, _, _ = _compare(rr, lists, n, scores=_score_bits(lists.shape, 2))
        if alpha == 0.3 and share == 0.3:
            assert all(not np.array_equal(t.positions, np.arange(n)) for t in traces)


def test_n_at_the_limit(gpu):
    from lkpy_amd import _native
    from lkpy_amd.reranking import FAIRReranker

    limit = _native.FAIR_MAX_N
    assert limit >= 1024
    with pytest.raises(ValueError, match=str(limit)):
        FAIRReranker(n=limit + 1)
    rng = np.random.default_rng(23)
    table = rng.random(4 * limit) < 0.3
    rr = _reranker(table, limit)
    lists = np.full((3, 3 * limit), -1, np.int32)
    lists[0] = rng.permutation(4 * limit)[:3 * limit]  # a row of 3 x limit
    lists[1, :5] = rng.permutation(4 * limit)[:5]  # a short row beside it
    lists[2, :limit] = rng.permutation(4 * limit)[:limit]
    scores = _score_bits(lists.shape, 8)
    traces, _, _ = _compare(rr, lists, limit, scores=scores)
    assert traces[0].constrained and not np.array_equal(traces[0].positions, np.arange(limit))
    _compare(rr, lists, limit - 1, scores=scores)


# ---- batch shapes ------------------------------------------------------------------------------------

def test_batch_shapes(gpu):
    import torch

    from lkpy_amd import _device as D

    rng = np.random.default_rng(29)
    table = rng.random(N_ITEMS) < 0.2
    n, L = 64, 70
    rr = _reranker(table, n)
    lists = np.argsort(rng.random((4099, N_ITEMS)), axis=1)[:, :L].astype(np.int32)
    cut = rng.integers(0, L + 1, size=len(lists))
    cut[:8] = [0, 1, 63, 64, 65, L, L, 0]
    for r, c in enumerate(cut):
        lists[r, c:] = -1
    scores = _score_bits(lists.shape, 4)
    scores[lists < 0] = np.nan
    _t, want, w_sc = _compare(rr, lists, n, scores=scores)  # B = 4099: a last workgroup of 3 rows
    for B in (1, 2, 3, 5, 6):
        _compare(rr, lists[:B], n, scores=scores[:B])
    # a row alone == the row in the batch, whatever stands beside it
    for r in (0, 2, 7, 8, 1234, 4098):
        a, b = rr.rerank_batch(lists[r:r + 1], scores[r:r + 1], n)
        assert np.array_equal(a[0], want[r]) and np.array_equal(_bits(b[0]), _bits(w_sc[r]))
    # explicit lengths == trailing padding
    a, b = rr.rerank_batch(lists, scores, n, lengths=cut.astype(np.int32))
    assert np.array_equal(a, want) and np.array_equal(_bits(b), _bits(w_sc))
    # a strided device view (rows 2 L apart) is read in place
    dev = D.device()
    wide = torch.full((64, 2 * L), -1, dtype=torch.int32, device=dev)
    wide[:, :L] = torch.from_numpy(lists[:64]).to(dev)
    wide_sc = torch.zeros((64, 2 * L), dtype=torch.float32, device=dev)
    wide_sc[:, :L] = torch.from_numpy(scores[:64]).to(dev)
    a, b = rr.rerank_batch(wide[:, :L], wide_sc[:, :L], n)
    assert np.array_equal(a, want[:64]) and np.array_equal(_bits(b), _bits(w_sc[:64]))
    # no rows, no columns
    a, b = rr.rerank_batch(np.zeros((0, L), np.int32), np.zeros((0, L), np.float32), n)
    assert a.shape == (0, n) and b.shape == (0, n)
    a, b = rr.rerank_batch(np.zeros((3, 0), np.int32), None, n)
    assert a.shape == (3, n) and (a == -1).all() and b is None


def test_state_pickles_without_the_device_copies(gpu):
    import pickle

    rr = _reranker(np.arange(N_ITEMS) % 3 == 0, 10)
    row = np.arange(40, dtype=np.int32).reshape(1, -1)
    before, _ = rr.rerank_batch(row)
    assert "fair" in rr.__dict__["_dev"]
    back = pickle.loads(pickle.dumps(rr))
    assert "_dev" not in back.__dict__
    assert np.array_equal(back.rerank_batch(row)[0], before)
    # retrained flags replace the cached table
    rr.protected_attributes = np.zeros(N_ITEMS, bool)
    assert list(rr.rerank_batch(row)[0][0]) == list(range(10))


# ---- the pipeline ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ml_run(gpu):
    "ml-latest-small + a user without history, flags at share 0.2, a trained ImplicitMF pipeline"
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import Dataset, Vocabulary, load_movielens_npz
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    ml = load_movielens_npz(GOLDEN / "ml_small.npz")
    lonely = int(ml.users.ids().max()) + 1
    users = Vocabulary(np.append(ml.users.ids(), lonely), "user")
    ds = Dataset(users, ml.items, ml._rows, ml._cols, dict(ml._attrs))
    ds.item_attrs["protected"] = np.random.default_rng(20).random(ds.item_count) < 0.2
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=16, epochs=2))
    pipe.train(ds, TrainingOptions(rng=42))
    uids = [int(u) for u in ml.users.ids()[::3][:198]] + [lonely, -5]  # + empty history, unknown
    return ds, pipe, uids, lonely


def _with_reranker(pipe, ds, n):
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.reranking import FAIRReranker

    both = Pipeline(pipe.name)
    both.nodes = dict(pipe.nodes)
    both.aliases, both.default = dict(pipe.aliases), pipe.default
    rr = FAIRReranker(n=n)
    rr.train(ds)
    both.add_reranker(rr)
    return both, rr


def _same_lists(got, want):
    assert np.array_equal(got.ids(), want.ids())
    if len(want) == 0:
        return
    assert np.array_equal(_bits(got.scores()), _bits(want.scores()))


def test_batch_recommend_with_a_reranker(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd import reranking_metrics as RM

    import diversity_restatement as DR

    ds, pipe, uids, lonely = ml_run
    n = 20
    both, rr = _with_reranker(pipe, ds, n)
    assert both.node("recommender").component is rr and pipe.node("recommender").component is not rr
    table, m = rr.protected_attributes, rr.m_list
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component

    # unchanged paths: without a reranker, batch.recommend is recommend_batch's arrays
    plain = batch.recommend(pipe, uids, n)
    p_i, p_s = scorer.recommend_batch(lookup.batch(np.asarray(uids)), n)
    for r, u in enumerate(uids):
        keep = p_i[r] >= 0
        assert np.array_equal(plain.lookup(u).numbers(vocabulary=scorer.items), p_i[r][keep])
        assert np.array_equal(_bits(plain.lookup(u).scores()), _bits(p_s[r][keep]))

    # batch.recommend == pipe.run per user, ids and score bits
    got = batch.recommend(both, uids, n)
    assert len(got) == len(uids)
    moved = 0
    for u in uids:
        one = both.run("recommender", query=u, n=n)
        _same_lists(got.lookup(u), one)
        moved += not np.array_equal(one.ids(), plain.lookup(u).ids())
    assert len(got.lookup(-5)) == 0 and moved > 0
    # ... == the restatement on the plain lists, and at another batch size
    w_i, w_s, _p, _t = R.rerank_rows(p_i, table, m, n, scores=p_s)
    small = batch.recommend(both, uids, n, batch_size=64)
    for r, u in enumerate(uids):
        keep = w_i[r] >= 0
        for out in (got, small):
            assert np.array_equal(out.lookup(u).numbers(vocabulary=scorer.items), w_i[r][keep])
            assert np.array_equal(_bits(out.lookup(u).scores()), _bits(w_s[r][keep]))

    # rerank_depth: the plain lists at depth 400, reranked down to n
    deep = batch.recommend(both, uids, n, rerank_depth=400)
    d_i, d_s = scorer.recommend_batch(lookup.batch(np.asarray(uids)), 400)
    plain400 = batch.recommend(pipe, uids, 400)
    w_i, w_s, _p, traces = R.rerank_rows(d_i, table, m, n, scores=d_s)
    assert sum(t.constrained for t in traces) >= len(uids) - 2
    differ = 0
    for r, u in enumerate(uids):
        keep = w_i[r] >= 0
        assert np.array_equal(plain400.lookup(u).numbers(vocabulary=scorer.items),
                              d_i[r][d_i[r] >= 0])
        assert np.array_equal(deep.lookup(u).numbers(vocabulary=scorer.items), w_i[r][keep])
        assert np.array_equal(_bits(deep.lookup(u).scores()), _bits(w_s[r][keep]))
        differ += not np.array_equal(deep.lookup(u).ids(), got.lookup(u).ids())
    assert differ > 0  # depth gave the reranker items to promote
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(both, uids, n, rerank_depth=n - 1)
    with pytest.raises(ValueError, match="exceeds configured"):
        batch.recommend(both, uids, n + 1)

    # a reranker over ANOTHER item vocabulary cannot take the scorer's numbers: per user then
    from lkpy_amd.data import Dataset
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.reranking import FAIRReranker

    fewer = ds.items.ids()[50:]
    other_ds = Dataset.from_arrays([1, 1], fewer[:2], all_item_ids=fewer)
    other_ds.item_attrs["protected"] = np.random.default_rng(21).random(len(fewer)) < 0.2
    other = FAIRReranker(n=n)
    other.train(other_ds)
    odd = Pipeline()
    odd.nodes, odd.aliases, odd.default = dict(pipe.nodes), dict(pipe.aliases), pipe.default
    odd.add_reranker(other)
    odd_out = batch.recommend(odd, uids[:6], n)
    for u in uids[:6]:
        _same_lists(odd_out.lookup(u), odd.run("recommender", query=u, n=n))

    # how far the reranker moved the lists: the device metrics == their restatements
    lip = RM.least_item_promoted_collection(plain400, deep, n=n)
    rbo = RM.rank_biased_overlap_collection(plain400, deep, n=n)
    assert len(lip) == len(rbo) == len(uids)
    for u in uids:
        ref, il = plain400.lookup(u).ids(), deep.lookup(u).ids()
        want_lip = DR.lip(ref, il, n)
        assert lip[u] == want_lip or (np.isnan(lip[u]) and np.isnan(want_lip)), u
        assert rbo[u] == DR.rbo(ref, il, n), u
    assert lip.max() > 0 and rbo.min() < 1


def test_stochastic_ranker_then_reranker(gpu, ml_run):
    from lkpy_amd import batch
    from lkpy_amd.pipeline import Pipeline
    from lkpy_amd.stochastic import StochasticTopNRanker

    ds, pipe, uids, lonely = ml_run
    n = 20
    scorer = pipe.node("scorer").component

    def sampled():
        p = Pipeline()
        p.nodes = {k: v for k, v in pipe.nodes.items() if k != "ranker"}
        p.aliases, p.default = dict(pipe.aliases), pipe.default
        p.add_component("ranker", StochasticTopNRanker(rng=(31, "user"), scale=4.0),
                        items="scorer", n="n", query="history-lookup")
        return p

    base = sampled()
    both, rr = _with_reranker(sampled(), ds, n)
    table, m = rr.protected_attributes, rr.m_list
    users = uids[:40] + uids[-2:]
    plain = batch.recommend(base, users, n)
    got = batch.recommend(both, users, n)
    moved = 0
    for u in users:
        ref = plain.lookup(u)
        row = ref.numbers(vocabulary=scorer.items).reshape(1, -1)
        w_i, w_s, _p, _t = R.rerank_rows(row, table, m, n, scores=ref.scores().reshape(1, -1),
                                         lengths=[len(ref)])
        k = len(ref)
        assert np.array_equal(got.lookup(u).numbers(vocabulary=scorer.items), w_i[0, :k])
        assert np.array_equal(_bits(got.lookup(u).scores()), _bits(w_s[0, :k]))
        moved += not np.array_equal(w_i[0, :k], row[0])
    assert moved > 0
    many_plain = batch.recommend_samples(base, users[:12], n, 3)
    many = batch.recommend_samples(both, users[:12], n, 3)
    assert many.key_fields == ("user_id", "sample") and len(many) == 36
    for (u, s), il in many:
        ref = many_plain.lookup(u, s)
        w_i, w_s, _p, _t = R.rerank_rows(ref.numbers(vocabulary=scorer.items).reshape(1, -1),
                                         table, m, n, scores=ref.scores().reshape(1, -1),
                                         lengths=[len(ref)])
        assert np.array_equal(il.numbers(vocabulary=scorer.items), w_i[0, :len(ref)])
        assert np.array_equal(_bits(il.scores()), _bits(w_s[0, :len(ref)]))
        if s == 0:
            _same_lists(il, got.lookup(u))
    with pytest.raises(ValueError, match="rerank_depth"):
        batch.recommend(both, users, n, rerank_depth=400)
