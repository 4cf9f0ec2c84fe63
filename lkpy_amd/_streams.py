"""
The random streams of the components that draw on the device (``StochasticTopNRanker``,
``RandomSelector``): an ``rng`` spec -> a 64-bit seed and one 64-bit *stream* per ranked row.
The draws themselves are defined in ``lkpy_amd.stochastic`` (module docstring) and DESIGN.md
section 4.18; NumPy only.
"""

from __future__ import annotations

from hashlib import md5

import numpy as np

_MASK64 = (1 << 64) - 1


def _bytes_stream(key: bytes) -> int:
    words = np.frombuffer(md5(key).digest(), np.int32)
    return abs(int(np.bitwise_xor.reduce(words)))


def user_stream(user_id) -> int | None:
    "The stream of a user id (``lkpy_amd.stochastic``); None for an id that cannot give one."
    if isinstance(user_id, (int, np.integer)):
        return int(user_id) & _MASK64
    if isinstance(user_id, str):
        return _bytes_stream(user_id.encode("utf8"))
    if isinstance(user_id, (bytes, np.bytes_)):
        return _bytes_stream(bytes(user_id))
    return None


def _seed_state(seed) -> int:
    "64 bits of a seed: SeedSequence(seed).generate_state(1, uint64)"
    if isinstance(seed, np.random.Generator):
        seed = seed.bit_generator
    if isinstance(seed, np.random.BitGenerator):
        return int(seed.random_raw()) & _MASK64
    if not isinstance(seed, np.random.SeedSequence):
        seed = np.random.SeedSequence(seed)
    return int(seed.generate_state(1, np.uint64)[0])


def parse_rng(spec) -> tuple[int, bool]:
    "An ``rng`` spec (random.py:315-349) -> (64-bit seed, streams by user id?)"
    if isinstance(spec, str):
        if spec != "user":
            raise ValueError(f"unrecognized rng specification {spec!r}")
        return _seed_state(None), True
    if isinstance(spec, tuple):
        if len(spec) != 2 or spec[1] != "user":
            raise ValueError(f"unrecognized key in rng specification {spec!r}")
        return _seed_state(spec[0]), True
    return _seed_state(spec), False


class RowStreams:
    "``seed``, ``by_user``, the call counter and :meth:`streams` of a component with an ``rng``."

    def _init_streams(self, rng) -> None:
        self.seed, self.by_user = parse_rng(rng)
        self.calls = 0

    def streams(self, user_ids, count: int | None = None) -> np.ndarray:
        """
        The uint64 streams of one call's rows: ``user_ids`` per row (None: ``count`` rows without
        ids).  Counts as one call.
        """
        n = len(user_ids) if user_ids is not None else int(count)
        out = (np.uint64(self.calls << 32) | np.arange(n, dtype=np.uint64))
        self.calls = (self.calls + 1) & 0xFFFFFFFF
        if self.by_user and user_ids is not None:
            if isinstance(user_ids, np.ndarray) and user_ids.dtype.kind in "iu":
                out = user_ids.astype(np.int64).view(np.uint64) if user_ids.dtype.kind == "i" \
                    else user_ids.astype(np.uint64)
            else:  # id by id: strings, bytes, a list of mixed ids
                ids = user_ids.tolist() if isinstance(user_ids, np.ndarray) and \
                    user_ids.dtype.kind != "O" else user_ids
                for i, u in enumerate(ids):
                    s = None if u is None else user_stream(u)
                    if s is not None:
                        out[i] = s
        return np.ascontiguousarray(out, dtype=np.uint64)
