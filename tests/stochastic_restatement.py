"""
NumPy restatement of the stochastic ranker's arithmetic, for the tests: Philox4x32-10, the uniform
the device kernel defines, the reference's ``_compute_keys``
(src/lenskit/stochastic/_ranker.py:119-156) in float64 fed those uniforms, and the log-domain key
``g = max(log w, log FLT_MIN) - log(-log u)`` in float64 and in float32.
"""

from __future__ import annotations

import numpy as np

TINY = float(np.finfo(np.float32).smallest_normal)
LOG_TINY = float(np.log(np.float64(TINY)))
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    "``counter``: uint32 [..., 4]; ``key``: (k0, k1) -> uint32 [..., 4]"
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _32) ^ c[3] ^ np.uint64(k1),
             p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def random_bits(seed: int, stream: int, sample: int, n_items: int) -> np.ndarray:
    "the random word of each of ``n_items`` items: counter (item >> 2, sample, stream), word item & 3"
    nq = (n_items + 3) // 4
    ctr = np.empty((nq, 4), np.uint32)
    ctr[:, 0] = np.arange(nq, dtype=np.uint32)
    ctr[:, 1] = sample
    ctr[:, 2] = stream & 0xFFFFFFFF
    ctr[:, 3] = (stream >> 32) & 0xFFFFFFFF
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return words.reshape(-1)[:n_items]


def uniform(bits) -> np.ndarray:
    "u = ((b >> 9) + 0.5) 2^-23 as float64 (an odd 24-bit integer times 2^-24: float32 holds it too)"
    return ((np.asarray(bits, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def weights64(scores, transform, scale) -> np.ndarray:
    "the weights of the reference's transforms, float64, from the valid scores"
    x = np.asarray(scores, np.float64) * float(scale)
    if transform == "softmax":
        e = np.exp(x - x.max())
        return e / e.sum()
    if transform == "linear":
        lo, hi = x.min(), x.max()
        if hi - lo > 0:
            t = (x - lo) / (hi - lo)
            if t.sum() > 0:
                return t / t.sum()
        return np.full(len(x), 1.0 / len(x))
    return x


def reference_keys(scores, transform, scale, u) -> np.ndarray:
    "``_compute_keys``: log(u) / max(w, tiny), float64"
    return np.log(u) / np.maximum(weights64(scores, transform, scale), TINY)


def log_weights64(scores, transform, scale) -> np.ndarray:
    x = np.asarray(scores, np.float64) * float(scale)
    if transform == "softmax":
        m = x.max()
        lw = (x - m) - np.log(np.exp(x - m).sum())
    else:
        w = weights64(scores, transform, scale)
        with np.errstate(divide="ignore", invalid="ignore"):
            lw = np.where(w >= TINY, np.log(np.maximum(w, TINY)), LOG_TINY)
    return np.maximum(lw, LOG_TINY)


def g64(scores, transform, scale, u) -> np.ndarray:
    return log_weights64(scores, transform, scale) - np.log(-np.log(u))


def g32(scores, transform, scale, u) -> np.ndarray:
    "the key in float32 arithmetic throughout (NumPy's float32 functions)"
    f = np.float32
    x = np.asarray(scores, f) * f(scale)
    if transform == "softmax":
        m = x.max()
        lw = (x - m) - np.log(np.exp(x - m).sum(dtype=f))
    else:
        if transform == "linear":
            lo, hi = x.min(), x.max()
            w = None
            if hi - lo > 0:
                t = (x - lo) / (hi - lo)
                tot = t.sum(dtype=f)
                if tot > 0:
                    w = t / tot
            if w is None:
                w = np.full(len(x), f(1.0) / f(len(x)), f)
        else:
            w = x
        lw = np.where(w >= f(TINY), np.log(np.maximum(w, f(TINY))), f(LOG_TINY))
    lw = np.maximum(lw.astype(f), f(LOG_TINY))
    u = np.asarray(u, f)
    nl = np.where(u > f(0.5), -np.log1p(-(f(1.0) - u)), -np.log(u)).astype(f)
    return (lw - np.log(nl)).astype(f)


def stable_descending(keys) -> np.ndarray:
    "indices of the non-NaN keys by descending key, ties by lower index"
    keys = np.asarray(keys)
    ok = np.flatnonzero(~np.isnan(keys))
    return ok[np.argsort(-keys[ok], kind="stable")]
