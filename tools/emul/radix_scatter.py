#!/usr/bin/env python3
"""
Lane-level NumPy model of one pass of the stable LSD radix sort (csrc/radix_sort.h): the index
arithmetic of ``rs_scatter_kernel`` -- the eight-ballot ``peers`` mask and ``rank`` of a key inside
its 64-key chunk, the uint16 per-(chunk, digit) count table that one thread per digit turns into
running offsets, the four-per-lane wave scan of ``tile_start``, the uint16 ``pos``, the digit-major
reorder through LDS and the global destination from ``goff`` -- and a plain model of
``rs_hist_kernel`` / ``rs_rowsum_kernel`` / ``rs_scan_kernel`` with the 256-wide trips of the scan
and its ``carry``.  Every narrow type of the kernel (unsigned short table, rank and pos) is narrow
here too, so an overflow there would show.

A tile is held as [CHUNKS, 64] arrays: position p = i * THREADS + t of the kernel is chunk
i * 4 + w, lane t & 63, i.e. p = chunk * 64 + lane; a ballot is one uint64 per chunk.

    python tools/emul/radix_scatter.py     # checks passes and chained sorts against a stable sort
"""
import numpy as np

THREADS, ITEMS, RADIX, W = 256, 16, 256, 64
TILE = THREADS * ITEMS
CHUNKS = TILE // W

_LANE = np.arange(W, dtype=np.uint64)
_LT = (np.uint64(1) << _LANE) - np.uint64(1)  # lanes below this one


def tiles_of(n):
    return (n + TILE - 1) // TILE


def digit_of(key, shift, mask):
    "(unsigned)(key >> shift) & mask"
    return ((key >> key.dtype.type(shift)) & key.dtype.type(0xffffffff)).astype(np.uint32) \
        & np.uint32(mask)


def ballot(pred):
    "__builtin_amdgcn_ballot_w64 of every chunk: [CHUNKS, 64] bool -> [CHUNKS, 1] uint64"
    return np.bitwise_or.reduce(pred.astype(np.uint64) << _LANE, axis=1, keepdims=True)


def hist_model(keys, shift, mask):
    "rs_hist_kernel: hist[digit][tile], digit-major"
    n, n_tiles = len(keys), tiles_of(len(keys))
    hist = np.zeros((RADIX, n_tiles), np.uint64)
    for tile in range(n_tiles):
        h = np.zeros(RADIX, np.uint32)
        base = tile * TILE
        for i in range(ITEMS):
            idx = base + i * THREADS + np.arange(THREADS)
            idx = idx[idx < n]
            np.add.at(h, digit_of(keys[idx], shift, mask), np.uint32(1))
        hist[:, tile] = h
    return hist


def rowsum_model(hist):
    "rs_rowsum_kernel: thread t sums row[t], row[t + 256], ...; then the tree over the 256 parts"
    n_tiles = hist.shape[1]
    part = np.zeros((RADIX, THREADS), np.uint64)
    for t in range(min(THREADS, n_tiles)):
        part[:, t] = hist[:, t::THREADS].sum(axis=1, dtype=np.uint64)
    w = THREADS // 2
    while w > 0:
        part[:, :w] += part[:, w:2 * w]
        w >>= 1
    return part[:, 0].copy()


def scan_model(hist, total):
    """rs_scan_kernel, all 256 blocks at once ([block, thread]): carry = the totals of the smaller
    digits; then trips of 256 tiles, Hillis-Steele inclusive scan, row[i] = carry + sh[t] - v"""
    n_tiles = hist.shape[1]
    t = np.arange(THREADS)
    d = np.arange(RADIX)[:, None]
    sh = np.where(t[None, :] < d, total[None, :], np.uint64(0)).astype(np.uint64)
    w = THREADS // 2
    while w > 0:
        sh[:, :w] += sh[:, w:2 * w]
        w >>= 1
    carry = sh[:, 0].copy()
    out = hist.copy()
    trips = 0
    for i0 in range(0, n_tiles, THREADS):
        i = i0 + t
        live = i < n_tiles
        v = np.zeros((RADIX, THREADS), np.uint64)
        v[:, live] = out[:, i[live]]
        sh = v.copy()
        off = 1
        while off < THREADS:
            add = np.zeros_like(sh)
            add[:, off:] = sh[:, :-off]
            sh = sh + add
            off <<= 1
        base = carry
        out[:, i[live]] = (base[:, None] + sh - v)[:, live]
        carry = base + sh[:, THREADS - 1]
        trips += 1
    return out, trips


def wave_scan_tile_start(tile_start):
    "lanes 0 .. 63, four totals each: in-lane running sums, shfl_up scan of the lane sums"
    lane = np.arange(W)
    a = np.zeros((4, W), np.uint32)
    s = np.zeros(W, np.uint32)
    for j in range(4):
        s = s + tile_start[1 + lane * 4 + j]
        a[j] = s
    incl = s.copy()
    off = 1
    while off < W:
        o = np.zeros(W, np.uint32)
        o[off:] = incl[:-off]  # __shfl_up(incl, off, 64); lanes below `off` keep their own
        incl = np.where(lane >= off, incl + o, incl)
        off <<= 1
    before = incl - s
    out = tile_start.copy()
    for j in range(4):
        out[1 + lane * 4 + j] = before + a[j]
    return out


def scatter_tile(keys, vals, shift, mask, goff, keys_out, vals_out):
    "rs_scatter_kernel for one tile of tile_n <= 4096 pairs; goff[digit] = offs[digit][tile]"
    tile_n = len(keys)
    assert 0 < tile_n <= TILE
    key = np.zeros(TILE, keys.dtype)
    val = np.zeros(TILE, vals.dtype)
    key[:tile_n], val[:tile_n] = keys, vals
    key, val = key.reshape(CHUNKS, W), val.reshape(CHUNKS, W)
    ok = (np.arange(TILE) < tile_n).reshape(CHUNKS, W)
    dig = digit_of(key, shift, mask)

    # lanes of the chunk with the same digit: eight ballots
    peers = np.broadcast_to(ballot(ok), (CHUNKS, W)).copy()
    for b in range(8):
        bit = ((dig >> np.uint32(b)) & np.uint32(1)).astype(bool)
        m = ballot(bit)
        peers &= np.where(bit, m, ~m)
    below = peers & _LT[None, :]
    rank = np.bitwise_count(below).astype(np.uint16)
    cnt = np.zeros((CHUNKS, RADIX), np.uint16)
    first = ok & (below == 0)  # the first lane of its digit in the chunk writes the count
    c_of = np.broadcast_to(np.arange(CHUNKS)[:, None], (CHUNKS, W))
    cnt[c_of[first], dig[first]] = np.bitwise_count(peers[first]).astype(np.uint16)

    # digit t: counts -> running offsets over the chunks (stored as unsigned short)
    run = np.zeros(RADIX, np.uint32)
    for c in range(CHUNKS):
        v = cnt[c].astype(np.uint32)
        cnt[c] = run.astype(np.uint16)
        run = run + v
    tile_start = np.zeros(RADIX + 1, np.uint32)
    tile_start[1:] = run
    tile_start = wave_scan_tile_start(tile_start)

    pos = (tile_start[dig] + cnt[c_of, dig].astype(np.uint32) + rank.astype(np.uint32)) \
        .astype(np.uint16)
    skey = np.zeros(TILE, keys.dtype)
    sval = np.zeros(TILE, vals.dtype)
    written = np.zeros(TILE, np.int32)
    np.add.at(written, pos[ok].astype(np.int64), 1)
    assert (written[:tile_n] == 1).all() and not written[tile_n:].any()  # a permutation of the tile
    skey[pos[ok]] = key[ok]
    sval[pos[ok]] = val[ok]

    p = np.arange(tile_n)
    k = skey[:tile_n]
    d = digit_of(k, shift, mask)
    dst = goff[d] + (p - tile_start[d].astype(np.int64)).astype(np.uint32).astype(np.uint64)
    keys_out[dst.astype(np.int64)] = k
    vals_out[dst.astype(np.int64)] = sval[:tile_n]


def radix_pass(keys, vals, shift, mask):
    "hist, rowsum, scan, scatter: one stable pass over digit bits [shift, shift + 8) & mask"
    n = len(keys)
    hist = hist_model(keys, shift, mask)
    offs, _trips = scan_model(hist, rowsum_model(hist))
    keys_out, vals_out = np.zeros_like(keys), np.zeros_like(vals)
    for tile in range(tiles_of(n)):
        lo, hi = tile * TILE, min(n, (tile + 1) * TILE)
        scatter_tile(keys[lo:hi], vals[lo:hi], shift, mask, offs[:, tile], keys_out, vals_out)
    return keys_out, vals_out


def pass_plan(begin_bit, end_bit):
    "radix_sort_pairs: (shift, mask, to_out) of every pass; the last pass writes the out pair"
    passes = max(1, (end_bit - begin_bit + 7) // 8)
    plan = []
    for p in range(passes):
        shift = begin_bit + 8 * p
        left = end_bit - shift
        bits = (left if left > 0 else 8) if left < 8 else 8
        plan.append((shift, (1 << bits) - 1, ((passes - 1 - p) & 1) == 0))
    return plan


def radix_sort_pairs(keys, vals, begin_bit, end_bit):
    plan = pass_plan(begin_bit, end_bit)
    assert plan[-1][2] and all(a[2] != b[2] for a, b in zip(plan, plan[1:]))  # ping-pong ends in out
    for shift, mask, _to_out in plan:
        keys, vals = radix_pass(keys, vals, shift, mask)
    return keys, vals


def stable_by_digit(keys, vals, shift, mask):
    order = np.argsort(digit_of(keys, shift, mask), kind="stable")
    return keys[order], vals[order]


def main():
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 3 * TILE + 5):
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        vals = np.arange(n, dtype=np.uint32)
        for shift, mask in ((0, 255), (8, 255), (24, 1)):
            got = radix_pass(keys, vals, shift, mask)
            want = stable_by_digit(keys, vals, shift, mask)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, shift)
    n = 2 * TILE + 77
    keys = rng.integers(0, 1 << 41, n, dtype=np.uint64)
    keys[1::2] = keys[::2][: n // 2]  # equal keys: the values tell whether it is stable
    vals = np.arange(n, dtype=np.uint32)
    for end_bit in (32, 34, 41):
        k = keys & np.uint64((1 << end_bit) - 1)
        got = radix_sort_pairs(k, vals, 0, end_bit)
        order = np.argsort(k, kind="stable")
        assert np.array_equal(got[0], k[order]) and np.array_equal(got[1], vals[order]), end_bit
    print("radix_scatter model: single passes and chained sorts identical to a stable sort")


if __name__ == "__main__":
    main()
