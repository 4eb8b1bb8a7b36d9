"""Transciphering with the lookups done in the clear: the round loop of fhe_transcipher_begin / _next on TRIVIAL
ciphertexts (mask zero, body = value * delta), every PBS replaced by reading the table the ABI exports
(fhestr.transcipher_tables).  The init / gather / apply steps are passed in, so the same loop drives the host restatement
(csrc/transcipher.cpp) and, on a GPU, the kernels (GpuSteps).  EncryptedRun is the same loop on real ciphertexts, every lookup
level through Engine.apply_lookup_table, for the noise measurement of tests/test_gpu_transcipher.py.  The shapes the
transcipher tests share, and a restatement of the taps in Python, live here too."""
import numpy as np

import fhestr
import oracle as O

WARMUP_ROUNDS, STATE_ROWS, DATA_ROWS = 18, 192, 256
KEYSTREAM = 3                                   # row kind after the registers 0 = a, 1 = b, 2 = c

# (n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg_mod, carry_mod) with TOY_K1's stds.  Every one is accepted by
# the gate for both ciphers AND by Engine(P): the engine instantiates blind rotation for N = 2048 k = 1, N = 1024 k = 2 and
# N = 512 k = 3 at one level only, so those rows take a one-level decomposition the gate's relative budget lets through.
# The transcipher kernels see k N + 1, log2(msg_mod) and delta of a shape and nothing else.  W1, W2 and W4 have a sound
# margin (9.2 sigma at 54 nominal variances) and are decrypted; W8, R2049 and R2049K2 are for runs without cryptography only
# (W8: about 1 sigma; the two R2049 shapes are swamped by their decomposition's rounding).
_SHAPES = {
    "W1": (16, 1, 256, 10, 2, 4, 4, 2, 8),                 # 1 bit per block, 8 blocks per character
    "W2": (16, 1, 256, 10, 2, 4, 4, 4, 4),                 # TOY_K1
    "W4": (16, 1, 256, 10, 2, 4, 4, 16, 1),                # 4 bits
    "W8": (16, 3, 512, 20, 1, 4, 4, 256, 1),               # 8 bits: all 8 sources of an apply, all 20 tables; 1,537-word rows, k = 3
    "R2049": (16, 1, 2048, 12, 1, 4, 4, 4, 4),             # PARAM_MESSAGE_2_CARRY_2's row length: 1,024 pairs, four trips of 256 threads
    "R2049K2": (16, 2, 1024, 9, 1, 4, 4, 16, 1),           # the same length from k = 2, 4 bits
    "R1537": (16, 3, 512, 20, 1, 4, 4, 2, 8),              # 768 pairs: three trips; 1 bit
}
WIDTHS = ("W1", "W2", "W4", "W8")


def oracle_shape(name) -> "O.Params":
    return O.TOY_K1 if name == "W2" else O.Params(*_SHAPES[name], 1e-12, 1e-15, "TOY_TC_" + name)


def shape(name) -> "fhestr.Params":
    p = oracle_shape(name)
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod, p.lwe_std, p.glwe_std, p.name)


def margin(params, nu=54) -> float:
    """half a table box over the modelled spread of a lookup input of nu nominal variances, in sigmas"""
    m = fhestr.noise_model(params)
    return m["half_box"] / (nu * m["v_pbs"] + m["v_ks"] + m["v_ms"]) ** 0.5


def plain_blocks(params, s: bytes) -> np.ndarray:
    """The block values of a string by shifts and masks: block b of character j is bits [bits b, bits b + bits) of byte j."""
    bits = params.msg_mod.bit_length() - 1
    return np.array([(c >> (bits * b)) & (params.msg_mod - 1) for c in s for b in range(8 // bits)], dtype=np.int64)


# ---- the taps, restated from the ciphers' specifications (Trivium: De Canniere & Preneel; Kreyvium: Canteaut et al.) ----
_REG_LEN, _FIRST_TAP, _OWN_TAP = (93, 84, 111), (66, 69, 66), (69, 78, 87)


def sources(cipher, kind, t):
    """What the lookup input of row `kind` at step t sums: ([(register, step, coefficient)], key row or None)."""
    kreyvium = cipher == "kreyvium"
    if kind == KEYSTREAM:
        return [(reg, t - lag, 1) for reg in range(3) for lag in (_FIRST_TAP[reg], _REG_LEN[reg])], (t % 128 if kreyvium else None)
    src, key_row = (kind + 2) % 3, (t % 128 if kreyvium and kind == 0 else None)            # a <- c, b <- a, c <- b
    mul = 5 if key_row is not None else 4
    n = _REG_LEN[src]
    return [(src, t - (n - 2), mul), (src, t - (n - 1), mul), (src, t - _FIRST_TAP[src], 1), (src, t - n, 1), (kind, t - _OWN_TAP[kind], 1)], key_row


def ring_row(streams: int, s: int, kind: int, t: int) -> int:
    """Ring row of kind[t] of stream s, t >= -128: slot (round mod 4), streams back to back at the round's row count."""
    round = (t + 128) // 64 - 2
    return (round % 4) * streams * DATA_ROWS + s * (DATA_ROWS if round >= WARMUP_ROUNDS else STATE_ROWS) + kind * 64 + (t + 128) % 64


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

    def start(self, ivs):
        """The initial state alone: a caller that wants to see every round runs the warm-up itself through _round."""
        self.ivs, self.S = list(ivs), len(ivs)
        self.ring = self.steps.init(self.cipher, self.S, self.key, self.ivs)
        self.round = 0
        return self

    def begin(self, ivs):
        self.start(ivs)
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
        self.last_in, self.last_tables, self.last_out = v, tables.reshape(-1), looked_up.astype(np.int64)
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


class GpuSteps:
    """The same three steps through transcipher_init_kernel, transcipher_gather_kernel and transcipher_apply_kernel."""

    def __init__(self, eng):
        self.eng = eng

    def init(self, cipher, S, key, ivs):
        return self.eng.transcipher_init(cipher, S, key, ivs)

    def gather(self, cipher, S, round, rows, ring, key, ivs, data, m):
        return self.eng.transcipher_gather(cipher, S, round, rows, ring, key, ivs, data, m)

    def apply(self, cipher, S, round, ring, n_bytes, m, out):
        return self.eng.transcipher_apply(cipher, S, round, ring, n_bytes, m, out)


class EncryptedRun:
    """The round loop on real ciphertexts, one step at a time so that a test can look at every lookup input: init and gather
    through the kernels, the lookups through Engine.apply_lookup_table with the exported tables uploaded as accumulators
    (lut_ids[t] = the engine's index of table t), the result written into the round's ring slot as ks_pbs does."""

    def __init__(self, eng, cipher, key_cts, lut_ids):
        self.eng, self.p, self.cipher = eng, eng.params, cipher
        self.key, self.lut_ids = np.ascontiguousarray(key_cts, dtype=np.uint64), np.asarray(lut_ids, dtype=np.uint32)

    def begin(self, ivs):
        self.ivs, self.S, self.round = list(ivs), len(ivs), 0
        self.ring = self.eng.transcipher_init(self.cipher, self.S, self.key, self.ivs)
        return self

    def gather(self, rows, data=None, m=0):
        """-> (pbs_in (S * rows, big), table numbers (S * rows,)) of the coming round"""
        pbs_in, tables = self.eng.transcipher_gather(self.cipher, self.S, self.round, rows, self.ring, self.key, self.ivs, data, m)
        return pbs_in.reshape(-1, self.p.big_size), tables.reshape(-1)

    def lookup(self, pbs_in, tables):
        """-> the lookup outputs (S * rows, big), also written to the ring; the round is over"""
        out = self.eng.apply_lookup_table(pbs_in, self.lut_ids[tables])
        at = slot_words(self.p, self.S, self.round)
        self.ring[at: at + out.size] = out.reshape(-1)
        self.round += 1
        return out

    def rows(self, index):
        return self.ring.reshape(-1, self.p.big_size)[index]
