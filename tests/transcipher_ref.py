"""Transciphering with the lookups done in the clear: the round loop of fhe_transcipher_begin / _next on TRIVIAL
ciphertexts (mask zero, body = value * delta), every PBS replaced by reading the table the ABI exports
(fhestr.transcipher_tables).  The init / gather / apply steps are passed in, so the same loop drives the host restatement
(csrc/transcipher.cpp) and, on a GPU, the kernels."""
import numpy as np

import fhestr

WARMUP_ROUNDS, STATE_ROWS, DATA_ROWS = 18, 192, 256


def trivial(params, values) -> np.ndarray:
    rows = np.zeros((len(values), params.big_size), dtype=np.uint64)
    rows[:, -1] = np.asarray(values, dtype=np.uint64) * np.uint64(params.delta)
    return rows


def trivial_values(params, rows) -> np.ndarray:
    """The values of trivial ciphertexts; anything else is an assertion."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, params.big_size)
    assert not rows[:, :-1].any(), "a mask word is not zero"
    assert not (rows[:, -1] % np.uint64(params.delta)).any(), "a body is not a multiple of delta"
    return (rows[:, -1] // np.uint64(params.delta)).astype(np.int64)


def slot_words(params, streams: int, round: int) -> int:
    return (round % 4) * streams * DATA_ROWS * params.big_size


class ClearLookupRun:
    """begin(ivs) / next(data) with the lookups in the clear.  steps: an object with init(cipher, S, key, ivs),
    gather(cipher, S, round, rows, ring, key, ivs, data, m) -> (pbs_in, tables) and apply(cipher, S, round, ring, n_bytes, m, out)."""

    def __init__(self, params, cipher, key_bits, steps):
        self.p, self.cipher, self.steps = params, cipher, steps
        self.key = trivial(params, key_bits)
        self.tables = fhestr.transcipher_tables(params)
        self.max_input = 0

    def begin(self, ivs):
        self.ivs, self.S = list(ivs), len(ivs)
        self.ring = self.steps.init(self.cipher, self.S, self.key, self.ivs)
        self.round = 0
        for _ in range(WARMUP_ROUNDS):
            self._round(STATE_ROWS, None, 0)
        return self

    def _round(self, rows, data, m):
        p = self.p
        pbs_in, tables = self.steps.gather(self.cipher, self.S, self.round, rows, self.ring, self.key, self.ivs, data, m)
        v = trivial_values(p, pbs_in)
        assert v.max() < p.msg_mod * p.carry_mod
        self.max_input = max(self.max_input, int(v.max()))
        looked_up = self.tables[tables.reshape(-1), v]
        at = slot_words(p, self.S, self.round)
        self.ring[at: at + self.S * rows * p.big_size] = trivial(p, looked_up).reshape(-1)      # what ks_pbs writes: S x rows rows back to back
        self.round += 1

    def next(self, data):
        """data: one bytes object per stream -> (S, n_bytes * blocks_per_char) block values."""
        p, n = self.p, len(data[0])
        bpc = fhestr.blocks_per_char(p)
        out = np.full((self.S * n * bpc, p.big_size), np.uint64(2**64 - 1), dtype=np.uint64)     # every block must be written
        buf = np.frombuffer(b"".join(data), dtype=np.uint8)
        for m in range(-(-n // 8)):
            self._round(DATA_ROWS, buf, m)
            self.steps.apply(self.cipher, self.S, self.round - 1, self.ring, n, m, out)
        return trivial_values(p, out).reshape(self.S, n * bpc)


class HostSteps:
    def __init__(self, params):
        self.p = params

    def init(self, cipher, S, key, ivs):
        return fhestr.transcipher_init_host(self.p, cipher, S, key, ivs)

    def gather(self, cipher, S, round, rows, ring, key, ivs, data, m):
        return fhestr.transcipher_gather_host(self.p, cipher, S, round, rows, ring, key, ivs, data, m)

    def apply(self, cipher, S, round, ring, n_bytes, m, out):
        return fhestr.transcipher_apply_host(self.p, cipher, S, round, ring, n_bytes, m, out)
