"""GPU: run evaluation (``lkpy_amd.metrics``: lk_rank_stats / lk_ideal_gain / lk_predict_errors +
host composition) against the per-list restatement ``tests/metrics_restatement.py``.

Bars (derived, not tuned): the integer statistics and every metric that is a ratio of them are
bit-equal; NaN exactly where the restatement has NaN; a float64 sum metric is within relative
``(3 L + 4) * 2**-53`` of the restatement, L = kept list length (two orderings of a sum of <= L
non-negative doubles differ by at most 2 (L - 1) u, one more u per term for the AP quotient /
gain product, a few for the final division)."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import metrics_restatement as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
U = 2.0 ** -53
CUTS = (None, 1, 5, 20, 100)
N_ITEMS = 9125
N_TRUTH_ITEMS = 9000  # items 9000 .. 9124 are in no truth row


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def _metric_set():
    "(label, metric, restatement(recs, test, gains) -> value, exact?)"
    from lkpy_amd import metrics as M

    geo, log = M.GeometricRankWeight(0.85), M.LogRankWeight()
    wts = {"log": (log, R.log_weight, None), "geo": (geo, R.geometric_weight, 1 / (1 - 0.85))}
    out = []
    for n in CUTS:
        s = "" if n is None else f"@{n}"
        out += [
            (f"Hit{s}", M.Hit(n), lambda r, t, g, n=n: R.hit(r, t, n), True),
            (f"RecipRank{s}", M.RecipRank(n), lambda r, t, g, n=n: R.recip_rank(r, t, n), True),
            (f"Precision{s}", M.Precision(n), lambda r, t, g, n=n: R.precision(r, t, n), True),
            (f"Recall{s}", M.Recall(n), lambda r, t, g, n=n: R.recall(r, t, n), True),
            (f"AP{s}", M.AveragePrecision(n),
             lambda r, t, g, n=n: R.average_precision(r, t, n), False),
        ]
        for wn, (w, rw, ssum) in wts.items():
            out += [
                (f"DCG-{wn}{s}", M.DCG(n, weight=w),
                 lambda r, t, g, n=n, rw=rw: R.dcg(r, t, n, rw), False),
                (f"DCGg-{wn}{s}", M.DCG(n, weight=w, gain="rating"),
                 lambda r, t, g, n=n, rw=rw: R.dcg(r, t, n, rw, g), False),
                (f"NDCG-{wn}{s}", M.NDCG(n, weight=w),
                 lambda r, t, g, n=n, rw=rw: R.ndcg(r, t, n, rw), False),
                (f"NDCGg-{wn}{s}", M.NDCG(n, weight=w, gain="rating"),
                 lambda r, t, g, n=n, rw=rw: R.ndcg(r, t, n, rw, g), False),
                (f"RBP-{wn}{s}", M.RBP(n, weight=w),
                 lambda r, t, g, n=n, rw=rw, ss=ssum: R.rbp(r, t, n, rw, ss), False),
                (f"RBPn-{wn}{s}", M.RBP(n, weight=w, normalize=True),
                 lambda r, t, g, n=n, rw=rw, ss=ssum: R.rbp(r, t, n, rw, ss, True), False),
            ]
    return out


def _synthetic(ld: int, B: int = 4096, seed: int = 20261016):
    """
    B lists in 16 classes (list q is of class q % 16, 256 lists = 6.25 % each), built so that
    every branch is taken: returns (lists [B x ld] with -1, truth item arrays, gains arrays).
    """
    rng = np.random.default_rng(seed)
    lists = np.full((B, ld), -1, np.int32)
    truth, gains = [], []
    gain_values = np.arange(0.5, 5.01, 0.5).astype(np.float32)
    for q in range(B):
        c = q % 16
        nt = int(rng.integers(1, 60))
        if c == 4:
            nt = 0  # empty truth row
        elif c == 5:
            nt = int(rng.integers(ld + 50, ld + 200))  # truth longer than the list
        elif c == 6:
            nt = int(rng.integers(4100, 5000))  # truth row of more than 4096 items
        t = rng.choice(N_TRUTH_ITEMS, nt, replace=False).astype(np.int32)
        g = rng.choice(gain_values, nt).astype(np.float32)
        g[rng.random(nt) < 0.05] = np.nan
        g[rng.random(nt) < 0.05] = -1.0
        truth.append(t)
        gains.append(g)
        others = np.setdiff1d(np.arange(N_TRUTH_ITEMS, dtype=np.int32), t)
        L = ld
        if c == 8:
            L = (0, 1, 63, 64, 65, 100)[(q // 16) % 6]
        row = rng.choice(others, L, replace=False)
        if c == 0 or nt == 0:
            pass  # no hit
        elif c == 1:
            row[0] = t[0]  # hit at rank 1
        elif c == 10 and ld > 100:
            at = rng.choice(np.arange(64, L), min(3, nt), replace=False)
            row[at] = t[: len(at)]  # first hit beyond rank 64
        elif L:
            nh = int(min(rng.integers(1, 12), nt, L))
            at = rng.choice(L, nh, replace=False)
            row[at] = rng.choice(t, nh, replace=False)
        if c == 7:
            at = rng.choice(L, 10, replace=False)
            row[at] = rng.choice(np.arange(N_TRUTH_ITEMS, N_ITEMS), 10, replace=False)
        if c == 3:
            row[7] = row[3] = t[1 % nt]  # a repeated item, and it is a hit
        lists[q, :L] = row
        if c == 2:
            lists[q, rng.choice(np.arange(10, 50), 6, replace=False)] = -1  # -1 in the middle
    return lists, truth, gains


def _collections(lists, truth, gains, keys=None):
    from lkpy_amd.data import ItemListCollection, Vocabulary

    vocab = Vocabulary(np.arange(N_ITEMS, dtype=np.int64), "item")
    B = len(lists)
    keys = np.arange(1000, 1000 + B, dtype=np.int64) if keys is None else keys
    out = ItemListCollection.from_arrays(keys, lists, np.zeros(lists.shape, np.float32), vocab)
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([len(t) for t in truth], out=offsets[1:])
    test = ItemListCollection.from_ragged(
        keys, offsets, np.concatenate(truth).astype(np.int64),
        {"rating": np.concatenate(gains).astype(np.float32)})
    return out, test


def _check_frame(frame: pd.DataFrame, mset, lists, truth, gains, sample=None):
    "every list value of ``frame`` against the restatement; returns the restatement's frame"
    idx = range(len(lists)) if sample is None else sample
    want = {lbl: np.empty(len(idx)) for lbl, *_ in mset}
    kept = []
    for j, q in enumerate(idx):
        recs = lists[q][lists[q] >= 0]
        kept.append(len(recs))
        for lbl, _m, fn, _e in mset:
            want[lbl][j] = fn(recs, truth[q], gains[q])
    kept = np.asarray(kept)
    for lbl, _m, _fn, exact in mset:
        got = frame[lbl].to_numpy()[list(idx)]
        w = want[lbl]
        assert np.array_equal(np.isnan(got), np.isnan(w)), lbl
        if exact:
            assert np.array_equal(_bits(got), _bits(w)), lbl
        else:
            ok = ~np.isnan(w)
            err = np.abs(got[ok] - w[ok])
            bound = (3 * kept[ok] + 4) * U * np.abs(w[ok])
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
            print(f"{lbl}: worst error / bound = {worst:.3f}")
            assert np.all(err <= bound), (lbl, worst)
    return want


def _collector(mset):
    from lkpy_amd import metrics as M

    mc = M.MeasurementCollector()
    for lbl, m, _fn, _e in mset:
        mc.add_metric(m, lbl)
    return mc


@pytest.mark.parametrize("ld", [100, 300])
def test_synthetic_batch_every_branch(gpu, ld):
    lists, truth, gains = _synthetic(ld)
    B = len(lists)
    # the conditions the batch was built for, on the restatement's own output
    st = np.array([R.int_stats(l[l >= 0], t) for l, t in zip(lists, truth)])
    n_recs, n_hits, first = st[:, 0], st[:, 1], st[:, 2]
    nt = np.array([len(t) for t in truth])
    five = 0.05 * B
    assert (n_hits == 0).sum() >= five and (first == 1).sum() >= five
    if ld == 100:
        assert set((0, 1, 63, 64, 65, 100)) <= set(n_recs.tolist())
    else:
        assert (first > 64).sum() >= five
    middle = [(l[: np.flatnonzero(l >= 0)[-1] + 1] < 0).any() if (l >= 0).any() else False
              for l in lists]
    assert sum(middle) >= five
    assert sum(len(np.unique(l[l >= 0])) < (l >= 0).sum() for l in lists) >= five
    assert (nt == 0).sum() >= five and (nt > n_recs).sum() >= five and (nt > 4096).sum() >= five
    assert sum((l >= N_TRUTH_ITEMS).any() for l in lists) >= five

    mset = _metric_set()
    out, test = _collections(lists, truth, gains)
    # the kernel's integer statistics themselves, bit-equal, at every cutoff
    import torch

    from lkpy_amd import metrics as M

    ts = M.truth_state(test, out._lists.vocab)
    rows = ts.match({"user_id": np.asarray(out._lists.raw_keys)}, B)
    assert np.array_equal(rows, np.arange(B))
    raw = M._rank_pass([m for _l, m, _f, _e in mset], torch.from_numpy(lists).to(gpu), ts, rows,
                       nt.astype(np.int64), gpu)
    assert np.array_equal(raw.n_recs_all, n_recs)
    for n in CUTS:
        sn = np.array([R.int_stats(l[l >= 0], t, n) for l, t in zip(lists, truth)])
        assert np.array_equal(raw.n_recs(n), sn[:, 0]), n
        assert np.array_equal(raw.n_hits(n), sn[:, 1]), n
        assert np.array_equal(raw.first_hit(n), sn[:, 2]), n
    mc = _collector(mset)
    with pytest.warns(Warning):
        run = mc.measure_run(out, test)
    frame = run.list_metrics
    assert list(frame.index.names) == ["user_id"] and len(frame) == B
    _check_frame(frame, mset, lists, truth, gains)

    # the same call again: the same bits
    with pytest.warns(Warning):
        again = mc.measure_run(out, test).list_metrics
    for lbl, *_ in mset:
        assert np.array_equal(_bits(frame[lbl]), _bits(again[lbl])), lbl

    # seven of the lists as a batch of their own: the same bits
    pick = [6, 16 + 6, 3, 8, 5, 2, 4095] if ld == 100 else [6, 10, 26, 3, 5, 2, 4095]
    out7, test7 = _collections(lists[pick], [truth[q] for q in pick], [gains[q] for q in pick],
                               keys=np.arange(1000, 1000 + B)[pick])
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        small = mc.measure_run(out7, test7).list_metrics
    for lbl, *_ in mset:
        assert np.array_equal(_bits(small[lbl]), _bits(frame[lbl].to_numpy()[pick])), lbl


def test_empty_test_side_is_nan_for_every_metric_that_says_so(gpu):
    """Section 2's corner cases through ``measure_list`` (a batch of one) and through a
    collection whose every matched truth row is empty: NaN for Hit / RecipRank / RBP / DCG / NDCG
    / Recall, graded ones included -- the gain field is never looked at (_dcg.py:111-113,
    214-216); Precision 0, AveragePrecision NaN (the stated deviation)."""
    import warnings

    from lkpy_amd import metrics as M
    from lkpy_amd.data import ItemList, ItemListCollection

    recs = ItemList([5, 9, 2], ordered=True)
    empties = (ItemList([]), ItemList(item_ids=np.zeros(0, np.int64),
                                      rating=np.zeros(0, np.float32)))
    nan_ms = [M.Hit(), M.RecipRank(2), M.RBP(), M.RBP(normalize=True), M.Recall(), M.DCG(),
              M.NDCG(), M.NDCG(5), M.DCG(gain="rating"), M.NDCG(gain="rating"),
              M.NDCG(2, gain="rating", weight=M.GeometricRankWeight(0.5))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for empty in empties:
            for m in nan_ms:
                want = {M.Hit: R.hit, M.RecipRank: R.recip_rank, M.RBP: R.rbp, M.Recall: R.recall,
                        M.DCG: R.dcg, M.NDCG: R.ndcg}[type(m)](recs.ids(), [])
                assert np.isnan(want) and np.isnan(m.measure_list(recs, empty)), m.label
            assert M.Precision().measure_list(recs, empty) == R.precision(recs.ids(), []) == 0.0
            assert np.isnan(M.AveragePrecision().measure_list(recs, empty))
        # a non-empty test list that has the gain field still works next to them
        full = ItemList(item_ids=[9, 7], rating=np.array([4.0, 2.0], np.float32))
        got = M.NDCG(gain="rating").measure_list(recs, full)
        assert got == pytest.approx(R.ndcg(recs.ids(), [9, 7], gains=[4.0, 2.0]), rel=1e-15)
        with pytest.raises(KeyError):
            M.NDCG(gain="rating").measure_list(recs, ItemList([9, 7]))  # _dcg.py:119-120
        # a collection call in which no output list has test data, and one with empty rows only
        out = ItemListCollection(("user_id",))
        out.add(recs, 1)
        out.add(ItemList([4], ordered=True), 2)
        for test in (ItemListCollection(("user_id",)),
                     ItemListCollection.from_ragged(np.array([1, 2]), np.zeros(3, np.int64),
                                                    np.zeros(0, np.int64))):
            mc = M.MeasurementCollector()
            for m in nan_ms:
                mc.add_metric(m, f"m{len(mc.metric_names)}")
            frame = mc.measure_run(out, test).list_metrics
            assert frame.shape == (2, len(nan_ms)) and frame.isna().all().all()
        # an empty prediction list against a rated truth list: nothing scored, all missing
        il = ItemList(item_ids=np.zeros(0, np.int64), scores=np.zeros(0, np.float32))
        assert M.RMSE(missing_scores="ignore").measure_list(il, full) == (0.0, 0)
        with pytest.raises(ValueError, match="missing scores for 2 truth items"):
            M.RMSE().measure_list(il, full)


@pytest.fixture(scope="module")
def ml_ds():
    from lkpy_amd.data import load_movielens_npz

    return load_movielens_npz(GOLDEN / "ml_small.npz")


def _test_arrays(split):
    "the test lists of a split as (user ids, {user: (item ids, ratings)})"
    ll = split.test._lists
    users = np.asarray(ll.raw_keys)
    by_user = {}
    for i, u in enumerate(users.tolist()):
        lo, hi = int(ll.offsets[i]), int(ll.offsets[i + 1])
        by_user[u] = (ll.item_ids[lo:hi], ll.fields["rating"][lo:hi])
    return users, by_user


def _ml_metric_set():
    from lkpy_amd import metrics as M

    return [
        ("RecipRank", M.RecipRank(), lambda r, t, g: R.recip_rank(r, t), True),
        ("RBP", M.RBP(), lambda r, t, g: R.rbp(r, t), False),
        ("NDCG", M.NDCG(), lambda r, t, g: R.ndcg(r, t), False),
        ("Hit", M.Hit(), lambda r, t, g: R.hit(r, t), True),
        ("Recall", M.Recall(), lambda r, t, g: R.recall(r, t), True),
        ("Precision", M.Precision(), lambda r, t, g: R.precision(r, t), True),
        ("AveragePrecision", M.AveragePrecision(),
         lambda r, t, g: R.average_precision(r, t), False),
        ("NDCG@10", M.NDCG(10), lambda r, t, g: R.ndcg(r, t, 10), False),
        ("NDCG-rating", M.NDCG(gain="rating"), lambda r, t, g: R.ndcg(r, t, None, gains=g), False),
    ]


def _check_summary(summary: dict, want: dict, kept_max: int):
    "the collector's summary against the same NumPy calls over the restatement's list values"
    for lbl, vals in want.items():
        ref = R.value_stats(vals)
        assert summary[f"{lbl}.n"] == ref["n"], lbl
        ok = ~np.isnan(vals)
        delta = float(np.max((3 * kept_max + 4) * U * np.abs(vals[ok]), initial=0.0))
        for stat in ("mean", "median", "std"):
            got, w = summary[f"{lbl}.{stat}"], ref[stat]
            assert abs(got - w) <= delta + 8 * np.spacing(abs(w)), (lbl, stat, got, w)


def test_ml_small_end_to_end(gpu, ml_ds, monkeypatch):
    """ml-latest-small, 134 test users, ImplicitMF k = 50, 10 epochs, top-20, seeds 42: on the
    device the restatement reports 117 lists with a hit and 17 without, mean NDCG 0.182 (the CPU
    rehearsal with the oracle's ALS gave 111 / 23 and 112 / 22, NDCG@20 about 0.21); the guard
    against a vacuous pass stays at 10 of each."""
    import torch

    from lkpy_amd import batch
    from lkpy_amd import metrics as M
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.data import _LazyLists
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.splitting import SampleFrac, sample_users
    from lkpy_amd.training import TrainingOptions

    split = sample_users(ml_ds, 134, SampleFrac(0.2, rng=42), rng=42)
    users, by_user = _test_arrays(split)
    assert len(users) == 134
    pipe = topn_pipeline(ImplicitMFScorer(embedding_size=50, epochs=10))
    pipe.train(split.train, TrainingOptions(rng=42))
    recs = batch.recommend(pipe, users, 20)
    nums = recs._lists.nums
    ids = split.train.items.ids()
    lists = [ids[r[r >= 0]] for r in nums]
    truth = [by_user[u][0] for u in users.tolist()]
    gains = [by_user[u][1] for u in users.tolist()]

    built = []
    real_make = _LazyLists._make
    monkeypatch.setattr(_LazyLists, "_make",
                        lambda self, pos: built.append(pos) or real_make(self, pos))
    mset = _ml_metric_set()
    mc = _collector(mset)
    run = mc.measure_run(recs, split.test)
    assert not built, "the batched route built ItemLists"
    frame = run.list_metrics
    assert np.array_equal(frame.index.to_numpy(), users)

    idl = [np.asarray(l) for l in lists]
    pad = np.full((len(idl), 20), -1, np.int64)
    for q, l in enumerate(idl):
        pad[q, : len(l)] = l
    want = _check_frame(frame, mset, pad, truth, gains)
    hits = np.array([R.hit(l, t) for l, t in zip(idl, truth)])
    print(f"lists with a hit: {int((hits == 1).sum())}, without: {int((hits == 0).sum())}, "
          f"NDCG mean {np.nanmean(want['NDCG']):.4f}")
    assert (hits == 1).sum() >= 10 and (hits == 0).sum() >= 10
    _check_summary(run.summary_metrics, want, 20)

    # the device tensors of recommend_batch(..., device_output=True): same frame, bit for bit
    scorer = pipe.node("scorer").component
    lookup = pipe.node("history-lookup").component
    d_idx, d_sc = scorer.recommend_batch(lookup.batch(users), 20, device_output=True)
    assert isinstance(d_idx, torch.Tensor) and d_idx.is_cuda
    mc2 = mc.empty_copy()
    mc2.add_array_measurements(users, d_idx, split.test, vocabulary=scorer.items)
    assert not built
    f2 = mc2.list_metrics()
    assert np.array_equal(f2.index.to_numpy(), users)
    for lbl, *_ in mset:
        assert np.array_equal(_bits(f2[lbl]), _bits(frame[lbl])), lbl


def test_predictions_rmse_mae(gpu, ml_ds):
    from lkpy_amd import batch
    from lkpy_amd import metrics as M
    from lkpy_amd.knn import ItemKNNScorer
    from lkpy_amd.pipeline import predict_pipeline
    from lkpy_amd.splitting import SampleFrac, sample_users

    split = sample_users(ml_ds, 134, SampleFrac(0.2, rng=7), rng=7)
    users, by_user = _test_arrays(split)
    pipe = predict_pipeline(ItemKNNScorer(max_nbrs=20))
    pipe.train(split.train)
    preds = batch.predict(pipe, split.test)
    ll = preds._lists
    mc = M.MeasurementCollector()
    mc.add_metric(M.RMSE())
    mc.add_metric(M.MAE())
    run = mc.measure_run(preds, split.test)
    frame = run.list_metrics
    tot_sse = tot_sae = 0.0
    tot_n = 0
    truth_st = M.truth_state(split.test)
    stats = M._predict_pass(M.pack_collection(preds), truth_st,
                            truth_st.match({"user_id": users}, len(users)), gpu)
    want_rmse, want_mae = [], []
    for i, u in enumerate(users.tolist()):
        lo, hi = int(ll.offsets[i]), int(ll.offsets[i + 1])
        sse, sae, n, ms, mt = R.predict_errors(ll.item_ids[lo:hi], ll.fields["score"][lo:hi],
                                               *by_user[u])
        assert (stats["n"][i], stats["n_missing_score"][i], stats["n_missing_truth"][i]) == \
            (n, ms, mt), u
        assert ms == 0 and mt == 0
        assert abs(stats["sse"][i] - sse) <= n * 2.0 ** -52 * sse, (u, stats["sse"][i], sse)
        assert abs(stats["sae"][i] - sae) <= n * 2.0 ** -52 * sae, (u, stats["sae"][i], sae)
        tot_sse, tot_sae, tot_n = tot_sse + sse, tot_sae + sae, tot_n + n
        want_rmse.append(np.sqrt(sse / n))
        want_mae.append(sae / n)
    big = tot_n * 2.0 ** -52
    # list values: the sums' n 2^-52 plus the division's and the square root's rounding
    rel = (stats["n"] + 2) * 2.0 ** -52
    for lbl, w in (("RMSE", np.asarray(want_rmse)), ("MAE", np.asarray(want_mae))):
        assert np.all(np.abs(frame[lbl].to_numpy() - w) <= rel * w), lbl
    s = run.summary_metrics
    assert abs(s["RMSE.global"] - np.sqrt(tot_sse / tot_n)) <= big * s["RMSE.global"]
    assert abs(s["MAE.global"] - tot_sae / tot_n) <= big * s["MAE.global"]
    assert s["RMSE.n"] == len(users)
    print(f"RMSE global {s['RMSE.global']:.4f}  MAE global {s['MAE.global']:.4f}")

    # without the fallback the unscorable items stay NaN: the two dispositions
    bare = predict_pipeline(ItemKNNScorer(max_nbrs=20), fallback=False)
    bare.train(split.train)
    holes = batch.predict(bare, split.test)
    hl = holes._lists
    n_nan = [int(np.isnan(hl.fields["score"][int(hl.offsets[i]):int(hl.offsets[i + 1])]).sum())
             for i in range(len(users))]
    assert sum(n_nan) > 0
    first = next(c for c in n_nan if c)
    for cls in (M.RMSE, M.MAE):
        c = M.MeasurementCollector()
        c.add_metric(cls())
        with pytest.raises(ValueError, match=f"missing scores for {first} truth items"):
            c.measure_run(holes, split.test)
        c = M.MeasurementCollector()
        c.add_metric(cls(missing_scores="ignore"))
        got = c.measure_run(holes, split.test)
        assert got.summary_metrics[f"{cls.__name__}.n"] > 0
    # scored items the truth does not rate: test lists cut to their first halves
    from lkpy_amd.data import ItemListCollection

    tl = split.test._lists
    lens = np.diff(tl.offsets)
    keep = np.concatenate([np.arange(int(tl.offsets[i]), int(tl.offsets[i]) + int(lens[i]) // 2)
                           for i in range(len(lens))])
    off2 = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens // 2, out=off2[1:])
    half = ItemListCollection.from_ragged(np.asarray(tl.raw_keys), off2, tl.item_ids[keep],
                                          {"rating": tl.fields["rating"][keep]})
    extra = int(lens[0] - lens[0] // 2)
    c = M.MeasurementCollector()
    c.add_metric(M.RMSE())
    with pytest.raises(ValueError, match=f"missing truth for {extra} scored items"):
        c.measure_run(preds, half)
    c = M.MeasurementCollector()
    c.add_metric(M.RMSE(missing_truth="ignore"))
    assert c.measure_run(preds, half).summary_metrics["RMSE.n"] > 0
    # one list that carries its own ratings
    from lkpy_amd.data import ItemList

    il = ItemList(item_ids=[1, 2, 3], scores=[3.0, 4.5, 2.0],
                  rating=np.array([3.5, 4.0, 2.0], np.float32))
    assert M.RMSE()(il) == pytest.approx(np.sqrt((0.25 + 0.25) / 3), rel=1e-15)
    assert M.MAE()(il) == pytest.approx(1.0 / 3, rel=1e-15)


@pytest.mark.parametrize("which", ["als", "iknn"])
def test_quick_measure_model(gpu, ml_ds, which):
    from lkpy_amd import metrics as M
    from lkpy_amd.als import ImplicitMFScorer
    from lkpy_amd.knn import ItemKNNScorer

    if which == "als":
        res = M.quick_measure_model(ImplicitMFScorer(embedding_size=50, epochs=10), ml_ds, rng=42)
        names = ["RecipRank", "RBP", "NDCG", "Hit", "Recall"]
    else:
        res = M.quick_measure_model(ItemKNNScorer(max_nbrs=20), ml_ds, predicts_ratings=True,
                                    rng=42)
        names = ["RecipRank", "RBP", "NDCG", "Hit", "Recall", "RMSE", "MAE"]
    assert isinstance(res, M.RunAnalysisResult)
    summ = res.list_summary()
    assert list(summ.index) == names and list(summ.columns) == ["mean", "median", "std"]
    recs, split = res.outputs["recommendations"], res.outputs["split"]
    users, by_user = _test_arrays(split)
    assert len(users) == ml_ds.user_count // 5
    truth = [by_user[u][0] for u in users.tolist()]
    gains = [by_user[u][1] for u in users.tolist()]
    mset = [m for m in _ml_metric_set() if m[0] in names]
    frame = res.list_metrics(fill_missing=False)
    assert sorted(frame.index.tolist()) == sorted(users.tolist())
    frame = frame.loc[users]  # (``merge_from`` joins the two frames: the index comes back sorted)
    pad = np.full((len(users), 20), -1, np.int64)
    for q, (key, il) in enumerate(recs):  # (after the measurement: the lists may be built now)
        assert key.user_id == users[q]
        pad[q, : len(il)] = il.ids()
    want = _check_frame(frame, mset, pad, truth, gains)
    # per-list slack the bars allow: 0 for the ratio metrics, (3 L + 4) u |value| for the sums
    slack = {lbl: 0.0 if exact else float(np.nanmax((3 * 20 + 4) * U * np.abs(want[lbl])))
             for lbl, _m, _fn, exact in mset}
    if which == "iknn":
        # RMSE / MAE of the predictions it produced: per list and ``global``
        preds = res.outputs["predictions"]
        pl = preds._lists
        assert [int(k) for k in pl.raw_keys] == users.tolist()
        rmse, mae, rel = [], [], []
        tot_sse = tot_sae = 0.0
        tot_n = 0
        for i, u in enumerate(users.tolist()):
            lo, hi = int(pl.offsets[i]), int(pl.offsets[i + 1])
            sse, sae, n, ms, mt = R.predict_errors(pl.item_ids[lo:hi], pl.fields["score"][lo:hi],
                                                   *by_user[u])
            assert n > 0 and ms == 0 and mt == 0
            rmse.append(np.sqrt(sse / n))
            mae.append(sae / n)
            rel.append((n + 2) * 2.0 ** -52)  # the sums' n 2^-52, + division and square root
            tot_sse, tot_sae, tot_n = tot_sse + sse, tot_sae + sae, tot_n + n
        rel = np.asarray(rel)
        for lbl, w in (("RMSE", np.asarray(rmse)), ("MAE", np.asarray(mae))):
            got = frame[lbl].to_numpy()
            assert np.all(np.abs(got - w) <= rel * w), lbl
            want[lbl] = w
            slack[lbl] = float(np.max(rel * w))
        glob = res.global_metrics()
        big = (tot_n + 2) * 2.0 ** -52
        assert abs(glob["RMSE.global"] - np.sqrt(tot_sse / tot_n)) <= big * glob["RMSE.global"]
        assert abs(glob["MAE.global"] - tot_sae / tot_n) <= big * glob["MAE.global"]
        assert glob["RMSE.n"] == len(users) and glob["MAE.n"] == len(users)
    # list_summary: pandas' mean / median / std (ddof = 1) over list values that differ from the
    # restatement's by at most the slack: mean and median move by at most that, std by at most
    # sqrt(n / (n - 1)) times it; plus 8 ulp for the calls' own rounding
    assert set(want) == set(names)
    grow = np.sqrt(len(users) / (len(users) - 1))
    for lbl in names:
        ref = pd.Series(want[lbl])
        for stat, w in (("mean", ref.mean()), ("median", ref.median()), ("std", ref.std())):
            got = summ.loc[lbl, stat]
            assert abs(got - w) <= slack[lbl] * grow + 8 * np.spacing(abs(w)), (lbl, stat, got, w)
    print(summ.to_string())


def test_scale_ml25m_shape(gpu):
    from lkpy_amd import metrics as M
    from lkpy_amd import synth
    from lkpy_amd.data import ItemListCollection, Vocabulary

    mat = synth.ml25m_like()
    n_users, n_items = mat.shape
    rng = np.random.default_rng(20261016)
    indptr = mat.indptr.astype(np.int64)
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(n_users), lens)
    order = np.argsort(rows + rng.random(mat.nnz), kind="stable")  # a random order inside a row
    pos = np.arange(mat.nnz) - np.repeat(indptr[:-1], lens)
    take = order[pos < np.repeat(np.round(lens * 0.2).astype(np.int64), lens)]
    t_rows, t_items = rows[take], mat.indices[take].astype(np.int64)
    o2 = np.argsort(t_rows, kind="stable")
    t_rows, t_items = t_rows[o2], t_items[o2]
    offsets = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(t_rows, minlength=n_users), out=offsets[1:])
    ld = 100
    stride = n_items // ld
    lists = (np.arange(ld, dtype=np.int32) * stride)[None, :] + \
        rng.integers(0, stride, (n_users, ld), dtype=np.int32)  # distinct by construction
    lists = rng.permuted(lists, axis=1)
    vocab = Vocabulary(np.arange(n_items, dtype=np.int64), "item")
    keys = np.arange(n_users, dtype=np.int64)
    out = ItemListCollection.from_arrays(keys, lists, np.zeros(lists.shape, np.float32), vocab)
    test = ItemListCollection.from_ragged(keys, offsets, t_items, {})
    mset = [m for m in _metric_set() if "g-" not in m[0]]
    mc = _collector(mset)
    frame = mc.measure_run(out, test).list_metrics
    good = np.isin(keys[:, None] * n_items + lists, t_rows * n_items + t_items)
    n_test = np.diff(offsets)
    for n in CUTS:
        s = "" if n is None else f"@{n}"
        g = good if n is None else good[:, :n]
        hits = g.sum(axis=1)
        first = np.where(hits > 0, g.argmax(axis=1) + 1, 0)
        k = ld if n is None else min(n, ld)
        assert np.array_equal(_bits(frame[f"Hit{s}"]),
                              _bits(np.where(n_test == 0, np.nan, hits > 0)))
        assert np.array_equal(_bits(frame[f"Precision{s}"]), _bits(hits / k))
        with np.errstate(all="ignore"):
            rr = np.where(first > 0, 1.0 / np.maximum(first, 1), 0.0)
            assert np.array_equal(_bits(frame[f"RecipRank{s}"]),
                                  _bits(np.where(n_test == 0, np.nan, rr)))
            nrel = n_test if n is None else np.minimum(n_test, n)
            assert np.array_equal(_bits(frame[f"Recall{s}"]), _bits(hits / nrel))
    sample = np.sort(rng.choice(n_users, 2000, replace=False)).tolist()
    truth = {q: t_items[offsets[q]:offsets[q + 1]] for q in sample}
    _check_frame(frame, [m for m in mset if not m[3]], lists,
                 _Lookup(truth), _Lookup({q: None for q in sample}), sample=sample)
    print(f"lists with a hit: {int((good.any(axis=1)).sum())} of {n_users}")


class _Lookup:
    def __init__(self, d):
        self.d = d

    def __getitem__(self, q):
        return self.d[q]
