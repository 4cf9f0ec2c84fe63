"""GPU: ``lk_ragged_stochastic_keys`` / ``stochastic.rank_ragged`` against the panel path they
restate -- each segment scattered into a dense NaN row, ``D.stochastic_keys`` / ``rank_panel`` on
it -- and ``lk_bmf_finish_ragged`` against ``predict_history_batch``.  Every comparison is of bit
patterns; there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
# the issue's widths (2048 | 2049: one wave | four waves of panel threads) and one wide enough
# for 48 entries of one of 256 threads
WIDTHS = (1, 3, 4, 5, 2048, 2049, 4101, 12293)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _one_thread(width, rng):
    "every entry of panel thread c: the quads c, c + BLK, ... -- up to 48 entries"
    blk = 64 if width <= 2048 else 256
    c = int(rng.integers(0, min(blk, max(1, width // 4))))
    quads = np.arange(c, (width + 3) // 4, blk)[:12]
    cols = (quads[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    return cols[cols < width]


def _segments(width, rng):
    "(columns, scores) per segment of one width: the cases of the issue"
    def normal(cols):
        return rng.standard_normal(len(cols)).astype(np.float32) * 3

    segs = [np.zeros(0, np.int64), rng.integers(0, width, 1), np.array([0, width - 1][:width]),
            np.arange(width)]
    if width >= 4:
        q = 4 * int(rng.integers(0, width // 4))
        segs.append(np.arange(q, q + 4))
    segs.append(_one_thread(width, rng))
    segs.append(np.sort(rng.choice(width, min(width, 100), replace=False)))
    out = [(np.unique(c).astype(np.int32), None) for c in segs]
    out = [(c, normal(c)) for c, _ in out]
    nan_cols = np.sort(rng.choice(width, min(width, 5), replace=False)).astype(np.int32)
    out.append((nan_cols, np.full(len(nan_cols), np.nan, np.float32)))
    mixed_cols = np.sort(rng.choice(width, min(width, 40), replace=False)).astype(np.int32)
    mixed = normal(mixed_cols)
    mixed[::3] = [np.nan, np.inf, -np.inf][len(mixed) % 3]
    out.append((mixed_cols, mixed))
    return out


@pytest.fixture(scope="module")
def batch():
    "segments of every width mixed in one launch: (ptr, addr, scores, widths, streams)"
    rng = np.random.default_rng(99)
    cols, scores, widths = [], [], []
    for w in WIDTHS:
        for c, s in _segments(w, rng):
            cols.append(c), scores.append(s), widths.append(w)
    order = rng.permutation(len(cols))  # widths and cases interleaved
    cols, scores = [cols[i] for i in order], [scores[i] for i in order]
    widths = np.array(widths, np.int32)[order]
    ptr = np.zeros(len(cols) + 1, np.int64)
    np.cumsum([len(c) for c in cols], out=ptr[1:])
    streams = rng.integers(0, 2 ** 63, len(cols), dtype=np.int64).astype(np.uint64)
    streams[::2] |= np.uint64(0xDEAD_BEEF) << np.uint64(32)  # high 32 bits set
    streams[1::4] &= np.uint64(0xFFFF_FFFF)  # ... and clear
    return ptr, np.concatenate(cols), np.concatenate(scores), widths, streams


def _panel_reference(gpu, ptr, addr, scores, widths, streams, *, transform, scale, samples,
                     first_sample):
    "(keys [samples x total], stats [B x 4]) from the PANEL kernels on the scattered rows"
    import torch

    from lkpy_amd import _device as D

    keys = np.empty((samples, len(addr)), np.float32)
    stats = np.empty((len(widths), 4), np.float32)
    for w in np.unique(widths):
        rows = np.flatnonzero(widths == w)
        panel = np.full((len(rows), int(w)), np.nan, np.float32)
        for r, s in enumerate(rows):
            panel[r, addr[ptr[s]:ptr[s + 1]]] = scores[ptr[s]:ptr[s + 1]]
        d_panel = torch.from_numpy(panel).to(gpu)
        st = None
        for j in range(samples):
            k, st = D.stochastic_keys(d_panel, streams[rows], transform=transform, scale=scale,
                                      seed=SEED, sample=first_sample + j, stats=st)
            k = k.cpu().numpy()
            for r, s in enumerate(rows):
                keys[j, ptr[s]:ptr[s + 1]] = k[r, addr[ptr[s]:ptr[s + 1]]]
        stats[rows] = st.cpu().numpy()
    return keys, stats


CASES = {
    "softmax": dict(transform="softmax", scale=1.0, samples=1, first_sample=0),
    "linear": dict(transform="linear", scale=1.0, samples=1, first_sample=0),
    "none": dict(transform=None, scale=1.0, samples=1, first_sample=0),
    "softmax-half": dict(transform="softmax", scale=0.5, samples=1, first_sample=0),
    "linear-half": dict(transform="linear", scale=0.5, samples=1, first_sample=0),
    "softmax-samples": dict(transform="softmax", scale=1.0, samples=3, first_sample=2),
    "none-samples": dict(transform=None, scale=2.0, samples=3, first_sample=2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_keys_and_stats_are_the_panel_kernels(gpu, batch, case):
    import torch

    from lkpy_amd import _device as D

    ptr, addr, scores, widths, streams = batch
    assert D.ragged_stochastic_chunk() < 2048 <= np.diff(ptr).max()  # a segment over the chunk
    opts = CASES[case]
    want_keys, want_stats = _panel_reference(gpu, ptr, addr, scores, widths, streams, **opts)
    keys, stats, _p, _a = D.ragged_stochastic_keys(
        ptr, addr, torch.from_numpy(scores).to(gpu), widths, streams, seed=SEED, **opts)
    torch.cuda.synchronize()
    got_stats, got_keys = stats.cpu().numpy(), keys.cpu().numpy()
    bad = np.flatnonzero((_bits(got_stats) != _bits(want_stats)).any(axis=1))
    assert len(bad) == 0, (bad[:5], widths[bad[:5]], got_stats[bad[:5]], want_stats[bad[:5]])
    assert got_keys.shape == want_keys.shape
    assert np.array_equal(_bits(got_keys), _bits(want_keys))
    finite = np.isfinite(scores)
    assert np.isnan(got_keys[:, ~finite]).all() and not np.isnan(got_keys[:, finite]).any()


def test_linear_with_equal_scores(gpu, batch):
    "every weight 1/N: the uniform branch of the key pass"
    import torch

    from lkpy_amd import _device as D

    ptr, addr, scores, widths, streams = batch
    flat = np.where(np.isfinite(scores), np.float32(2.5), scores).astype(np.float32)
    opts = dict(transform="linear", scale=1.0, samples=2, first_sample=0)
    want_keys, want_stats = _panel_reference(gpu, ptr, addr, flat, widths, streams, **opts)
    keys, stats, _p, _a = D.ragged_stochastic_keys(
        ptr, addr, torch.from_numpy(flat).to(gpu), widths, streams, seed=SEED, **opts)
    assert np.array_equal(_bits(stats.cpu().numpy()), _bits(want_stats))
    assert np.array_equal(_bits(keys.cpu().numpy()), _bits(want_keys))


def test_a_segment_is_the_same_alone_and_in_a_batch(gpu):
    import torch

    from lkpy_amd import _device as D

    rng = np.random.default_rng(3)
    width = 4101
    cols = [np.sort(rng.choice(width, int(rng.integers(0, 700)), replace=False)).astype(np.int32)
            for _ in range(50)]
    ptr = np.zeros(51, np.int64)
    np.cumsum([len(c) for c in cols], out=ptr[1:])
    addr = np.concatenate(cols)
    scores = rng.standard_normal(len(addr)).astype(np.float32)
    streams = rng.integers(0, 2 ** 63, 50, dtype=np.int64).astype(np.uint64)
    opts = dict(transform="softmax", scale=1.5, seed=SEED, samples=2, first_sample=1)
    keys, stats, _p, _a = D.ragged_stochastic_keys(
        ptr, addr, torch.from_numpy(scores).to(gpu), np.full(50, width, np.int32), streams, **opts)
    keys, stats = keys.cpu().numpy(), stats.cpu().numpy()
    again, _s, _p, _a = D.ragged_stochastic_keys(
        ptr, addr, torch.from_numpy(scores).to(gpu), np.full(50, width, np.int32), streams, **opts)
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(keys))  # the same inputs: the same bits
    for s in (0, 17, 49):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        k1, s1, _p, _a = D.ragged_stochastic_keys(
            [0, hi - lo], addr[lo:hi], torch.from_numpy(scores[lo:hi]).to(gpu), [width],
            streams[s:s + 1], **opts)
        assert np.array_equal(_bits(k1.cpu().numpy()), _bits(keys[:, lo:hi]))
        assert np.array_equal(_bits(s1.cpu().numpy()[0]), _bits(stats[s]))


@pytest.mark.parametrize("n", [1, 10, 150, -1])
def test_rank_ragged_is_rank_panel(gpu, n):
    "the same items and the same key bits as ``rank_panel`` on the scattered panel"
    import torch

    from lkpy_amd.stochastic import rank_panel, rank_ragged

    rng = np.random.default_rng(21)
    width, B = 2049, 12
    lens = [0, 1, 5, 10, 11, 64, 65, 100, 140, 300, 1100, 2049]  # shorter and longer than n
    cols = [np.sort(rng.choice(width, m, replace=False)).astype(np.int32) for m in lens]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    addr = np.concatenate(cols)
    scores = rng.standard_normal(len(addr)).astype(np.float32)
    scores[rng.random(len(scores)) < 0.1] = np.nan
    scores[ptr[4]:ptr[5]] = 0.75  # equal scores still draw distinct keys
    streams = rng.integers(0, 2 ** 63, B, dtype=np.int64).astype(np.uint64)
    panel = np.full((B, width), np.nan, np.float32)
    for b in range(B):
        panel[b, cols[b]] = scores[ptr[b]:ptr[b + 1]]
    opts = dict(transform="softmax", scale=2.0, seed=SEED, samples=2, first_sample=0)
    want_i, want_k = rank_panel(torch.from_numpy(panel).to(gpu), streams, n, **opts)
    got_i, got_k = rank_ragged(ptr, addr, None, torch.from_numpy(scores).to(gpu),
                               np.full(B, width, np.int32), streams, n, **opts)
    assert got_i.shape == got_k.shape == (B, 2, max(lens) if n < 0 else n)
    w = got_i.shape[2]  # (the panel's lists are as wide as the row when n < 0)
    assert np.array_equal(got_i, want_i[:, :, :w])
    assert np.array_equal(_bits(got_k), _bits(want_k[:, :, :w]))
    assert (want_i[:, :, w:] == -1).all()
    valid = np.array([np.isfinite(scores[ptr[b]:ptr[b + 1]]).sum() for b in range(B)])
    assert np.array_equal((got_i[:, 0] >= 0).sum(axis=1), np.minimum(valid, w))
    # a payload of its own rides along instead of the addresses
    pay = np.arange(len(addr), dtype=np.int32) + 7
    own_i, own_k = rank_ragged(ptr, addr, pay, torch.from_numpy(scores).to(gpu),
                               np.full(B, width, np.int32), streams, n, **opts)
    assert np.array_equal(_bits(own_k), _bits(got_k))
    for b in range(B):
        keep = got_i[b, 0] >= 0
        at = ptr[b] + np.searchsorted(cols[b], got_i[b, 0][keep])
        assert np.array_equal(own_i[b, 0][keep], pay[at])


# ---- lk_bmf_finish_ragged -------------------------------------------------------------------------
@pytest.mark.parametrize("user_embeddings", [True, "prefer"])
def test_bmf_finish_ragged_is_predict_history_batch(gpu, user_embeddings):
    "fold-in (True) and stored (``prefer``) rows, an unknown user (invalid), an unknown item (NaN)"
    import torch

    from lkpy_amd import _device as D
    from lkpy_amd.als import BiasedMFScorer
    from lkpy_amd.data import Dataset
    from lkpy_amd.pipeline import topn_pipeline
    from lkpy_amd.training import TrainingOptions

    rng = np.random.default_rng(8)
    U, I = 40, 300
    mask = rng.random((U, I)) < 0.12
    mask[np.arange(U), rng.integers(0, I, U)] = True
    rows, cols = np.nonzero(mask)
    ds = Dataset.from_arrays(rows + 100, cols + 1000,
                             rng.integers(1, 11, len(rows)).astype(np.float32) / 2,
                             all_item_ids=np.arange(I) + 1000)
    pipe = topn_pipeline(BiasedMFScorer(features=8, epochs=2, user_embeddings=user_embeddings))
    pipe.train(ds, TrainingOptions(rng=5))
    scorer, lookup = pipe.node("scorer").component, pipe.node("history-lookup").component
    users = np.array([100, 117, 9999, 139, 101])  # 9999: nobody
    lens = [300, 0, 20, 7, 1]
    ptr = np.zeros(6, np.int64)
    np.cumsum(lens, out=ptr[1:])
    nums = np.concatenate([np.arange(300), rng.integers(0, I, 20), rng.integers(0, I, 7),
                           [5]]).astype(np.int32)
    nums[[3, 310, 322]] = -1  # unknown items
    hb = lookup.batch(users)
    d_ptr, d_nums = D.upload_targets(ptr, nums, gpu)
    want = scorer.predict_history_batch(hb, d_ptr, d_nums, h_tgt_ptr=ptr).cpu().numpy()

    def never(*a, **k):
        raise AssertionError("a dense panel was formed")

    # what a candidate route composes: ``_batch_operands``, the dense chain at the targets alone,
    # the finish -- no panel
    dense, D.score_dense = D.score_dense, never
    try:
        u, _mode, d_mode, ub, _hist, pending = scorer._batch_operands(hb)
        st = scorer._device_state()
        u_rows = torch.arange(u.shape[0], dtype=torch.int32, device=gpu)
        dots = D.score_candidates(u, st["Q"], scorer.config.embedding_size, u_rows, d_ptr,
                                  d_nums, ptr)
        got = D.bmf_finish_ragged(dots, d_mode, ub, scorer.bias.global_bias, st["item_biases"],
                                  d_ptr, d_nums, ptr)
        assert got is dots  # (in place)
        for plan in pending:
            plan.check_status()
        got = got.cpu().numpy()
    finally:
        D.score_dense = dense
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(got[[3, 310, 322]]).all() and np.isnan(got[ptr[2]:ptr[3]]).all()
    known = np.ones(len(nums), bool)
    known[[3, 310, 322]] = False
    known[ptr[2]:ptr[3]] = False
    assert np.isfinite(got[known]).all()
