"""
FunkSVD restated in Python and NumPy, the yardstick of ``tests/test_funksvd_host.py`` and
``tests/test_gpu_funksvd.py``.

``feature_epoch`` is ``FunkSVDTrainer::feature_epoch`` (src/accel/funksvd.rs:67-128) in Python
floats: every operation is one IEEE double operation rounded once, which is what the Rust does
(it contracts nothing).  ``levels`` / ``plan`` are the level schedule, ``feature_epoch`` takes an
``order`` to walk the samples by level, and ``train`` is the loop of ``FunkSVDScorer.train``
(src/lenskit/funksvd.py:141-190) around it.
"""
import numpy as np

INITIAL_VALUE = 0.1
NARROW = 64  # a level this wide or narrower is walked by one wave
STAGE = 2048  # the samples of one narrow run


def levels(users, items, n_users, n_items):
    "level(s) = 1 + max(level of u's previous sample, level of i's previous sample), from 0"
    last_u, last_i = [0] * n_users, [0] * n_items
    out = np.empty(len(users), np.int32)
    for s, (u, i) in enumerate(zip(users.tolist(), items.tolist())):
        l = max(last_u[u], last_i[i]) + 1
        last_u[u] = last_i[i] = l
        out[s] = l - 1
    return out


def plan(level):
    """(order, level_ptr, run_end) of a level assignment: the stable sort by level, the levels'
    offsets, and for a level in a run of levels of at most 64 samples -- extended level by level
    while the run holds at most 2048 samples -- one past the run's last level (the level itself
    otherwise)"""
    depth = int(level.max()) + 1 if len(level) else 0
    order = np.argsort(level, kind="stable").astype(np.int64)
    ptr = np.zeros(depth + 1, np.int64)
    np.cumsum(np.bincount(level, minlength=depth), out=ptr[1:])
    width = np.diff(ptr)
    run_end = np.empty(depth, np.int32)
    l = 0
    while l < depth:
        if width[l] > NARROW:
            run_end[l] = l
            l += 1
            continue
        e = l + 1
        while e < depth and width[e] <= NARROW and ptr[e + 1] - ptr[l] <= STAGE:
            e += 1
        run_end[l:e] = e
        l = e
    return order, ptr, run_end


def feature_epoch(users, items, ratings, est, ucol, icol, lr, reg, trail, rmin, rmax, order=None):
    """One epoch of one feature, ``ucol`` / ``icol`` (float32) updated in place, the samples in
    their own order or in ``order``.  Returns (sse summed in that order, samples clamped)."""
    walk = range(len(users)) if order is None else order.tolist()
    us, its = users.tolist(), items.tolist()
    rs, es = ratings.astype(np.float64).tolist(), est.astype(np.float64).tolist()
    f32 = np.float32
    sse, clamped = 0.0, 0
    for s in walk:
        u, i = us[s], its[s]
        ufv, ifv = float(ucol[u]), float(icol[i])
        pred = es[s] + ufv * ifv + trail
        if pred < rmin:
            pred, clamped = rmin, clamped + 1
        if pred > rmax:
            pred, clamped = rmax, clamped + 1
        error = rs[s] - pred
        sse += error * error
        ufd = (error * ifv - reg * ufv) * lr
        ifd = (error * ufv - reg * ifv) * lr
        ucol[u] = f32(ufv + ufd)
        icol[i] = f32(ifv + ifd)
    return sse, clamped


def train(users, items, ratings, est, n_users, n_items, k, epochs, lr, reg, rng_range=None,
          order=None):
    """funksvd.py:148-190 from the shuffled samples and their initial estimates.  Returns (user
    embeddings, item embeddings, sse [k x epochs], samples clamped)."""
    est = est.astype(np.float32).copy()
    uemb = np.full([n_users, k], INITIAL_VALUE, dtype=np.float32, order="F")
    iemb = np.full([n_items, k], INITIAL_VALUE, dtype=np.float32, order="F")
    rmin, rmax = rng_range if rng_range is not None else (-np.inf, np.inf)
    sse = np.zeros((k, epochs))
    clamped = 0
    for f in range(k):
        trail = INITIAL_VALUE * INITIAL_VALUE * (k - f - 1)
        for e in range(epochs):
            sse[f, e], c = feature_epoch(users, items, ratings, est, uemb[:, f], iemb[:, f], lr,
                                         reg, trail, rmin, rmax, order)
            clamped += c
        est = np.clip(est + uemb[users, f] * iemb[items, f], rmin, rmax)
        assert est.dtype == np.float32
    return uemb, iemb, sse, clamped


def initial_estimates(users, items, global_bias, item_biases, user_biases):
    "funksvd.py:142-146"
    est = np.full(len(users), global_bias, dtype=np.float32)
    if item_biases is not None:
        est += item_biases[items]
    if user_biases is not None:
        est += user_biases[users]
    return est


def rmse(sse, n):
    return np.sqrt(np.asarray(sse) / n)


def score(uvec, ivecs, global_bias, item_bias, user_bias):
    "funksvd.py:211-220 in float64: the inner products plus the three biases"
    return ivecs.astype(np.float64) @ uvec.astype(np.float64) + \
        (float(global_bias) + item_bias.astype(np.float64) + float(user_bias))


# ---- the cases the host and the device tests share -------------------------------------------
def _ratings_and_estimates(rng, n):
    "half-star ratings and float32 start estimates around their mean (some beyond 4.5)"
    ratings = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    est = (np.float32(ratings.mean()) + rng.normal(0.0, 0.6, n)).astype(np.float32)
    return ratings, est


def case_cross(n_users, n_items, seed, density=0.08):
    """(users, items, ratings, est), shuffled: random pairs, user 0 with every item, item 0 with
    every user, and two pairs that occur twice"""
    rng = np.random.default_rng(seed)
    mask = rng.random((n_users, n_items)) < density
    mask[0, :] = True
    mask[:, 0] = True
    u, i = np.nonzero(mask)
    twice = rng.choice(len(u), 2, replace=False)
    u, i = np.concatenate([u, u[twice]]), np.concatenate([i, i[twice]])
    shuf = rng.permutation(len(u))
    users, items = u[shuf].astype(np.int32), i[shuf].astype(np.int32)
    return (users, items, *_ratings_and_estimates(rng, len(users)))


MATCHING_WIDTHS = [65, 64, 63, 1, 1, 70, 1024, 1025, 2, 64]


def case_matchings(seed=9, size=1025):
    """(users, items, ratings, est, level): one matching over ``size`` users and items per entry
    of MATCHING_WIDTHS, stacked; ``level`` assigns matching j to level j.  (The shallowest
    schedule of these samples is another one: a level is at most twice as wide as the level
    before it.  Any schedule of matchings that keeps the sample order has the sequential bits.)"""
    rng = np.random.default_rng(seed)
    users = np.concatenate([rng.permutation(size)[:w] for w in MATCHING_WIDTHS]).astype(np.int32)
    items = np.concatenate([rng.permutation(size)[:w] for w in MATCHING_WIDTHS]).astype(np.int32)
    level = np.repeat(np.arange(len(MATCHING_WIDTHS)), MATCHING_WIDTHS).astype(np.int32)
    return (users, items, *_ratings_and_estimates(rng, len(users)), level)


def case_singletons(n_users=40000, n_items=50, seed=13):
    "(users, items, ratings, est): every user has one rating -- 160 KB of user column alone"
    rng = np.random.default_rng(seed)
    users = rng.permutation(n_users).astype(np.int32)
    items = rng.integers(0, n_items, n_users).astype(np.int32)
    return (users, items, *_ratings_and_estimates(rng, n_users))
