"""The LWE keyswitch written from its definition, in exact integers, and inputs that sit on the edges of its arithmetic
(test infrastructure; independent of oracle/ and of the engine).

    out = (0, ..., 0, body) - sum_{i, lv} digit(a_i, lv) * KSK[i][lv][:]            (mod 2^64)

(core_crypto/algorithms/lwe_keyswitch.rs:96-170) with the signed digits of the closest representable value of a_i, the
least significant level (level L) first (decomposer.rs:98-152, iter.rs:37-127): KSK[i][0] meets the digit of level L.

Two forms:
  * keyswitch_int: Python integers only, one multiplication at a time -- the definition, for small shapes;
  * ExactKeyswitch: the same sum as matrix products.  The key words are split into four 16-bit limbs, each limb's
    product  digits [B, rows] @ limb [rows, n + 1]  is taken in float64 -- every partial sum is an integer below
    max|digit| * 65535 * rows, exact while that stays below 2^53 (asserted) -- and the limb products recombine in wrapping
    uint64.  About a second for 1027 all-distinct LWEs of PARAM_MESSAGE_2_CARRY_2 (10240 x 743 key)."""
import numpy as np

from exact_pbs import decompose

U64 = np.uint64
M64 = (1 << 64) - 1


# ---- the definition, Python integers --------------------------------------------------------------------------------

def closest_representable_int(x, base_log, level):
    """decomposer.rs:98-118: x rounded to a multiple of 2^(64 - base_log * level), ties up, mod 2^64."""
    non_rep = 64 - base_log * level
    return ((((x >> (non_rep - 1)) + 1) >> 1) << non_rep) & M64


def decompose_int(x, base_log, level):
    """Signed digits of closest_representable(x), level `level` first (iter.rs:101-127): list of Python ints in
    [-B/2, B/2].  The carry out of level 1 is dropped (the reduction mod 2^64)."""
    state = closest_representable_int(x, base_log, level) >> (64 - base_log * level)
    B = 1 << base_log
    digits = []
    for _ in range(level):
        res = state & (B - 1)
        state >>= base_log
        carry = ((((res - 1) & M64) | state) & res) >> (base_log - 1)
        state += carry
        digits.append(res - (carry << base_log))
    return digits


def keyswitch_int(params, ksk, ct):
    """One big-key LWE -> small-key LWE, Python integers throughout."""
    in_dim, out_size, bl, L = params.k * params.N, params.n + 1, params.ks_base_log, params.ks_level
    ksk = np.asarray(ksk, dtype=U64).reshape(in_dim * L, out_size)
    out = [0] * out_size
    out[-1] = int(ct[in_dim])
    for i in range(in_dim):
        for lv, d in enumerate(decompose_int(int(ct[i]), bl, L)):
            if d:
                row = ksk[i * L + lv].tolist()
                for j in range(out_size):
                    out[j] -= d * row[j]
    return np.array([v & M64 for v in out], dtype=U64)


# ---- the same sum as exact float64 limb products -----------------------------------------------------------------------

LIMB_BITS = 16


class ExactKeyswitch:
    """keyswitch of whole batches under one key: ExactKeyswitch(params, ksk)(cts [B, k N + 1]) -> [B, n + 1]."""

    def __init__(self, params, ksk):
        self.in_dim, self.out_size = params.k * params.N, params.n + 1
        self.bl, self.L = params.ks_base_log, params.ks_level
        rows = self.in_dim * self.L
        # |digit| <= 2^(bl - 1), limb <= 65535: every partial sum of a limb product is an integer of magnitude below this
        self.bound = (1 << (self.bl - 1)) * ((1 << LIMB_BITS) - 1) * rows
        assert self.bound < 1 << 53, f"float64 limb products would round: {self.bound} >= 2^53"
        ksk = np.asarray(ksk, dtype=U64).reshape(rows, self.out_size)
        self.limbs = [((ksk >> U64(LIMB_BITS * j)) & U64((1 << LIMB_BITS) - 1)).astype(np.float64) for j in range(64 // LIMB_BITS)]

    def digits(self, cts):
        """[B, in_dim * L] int64, column i * L + lv = digit lv (level L first) of mask element i."""
        mask = np.ascontiguousarray(np.asarray(cts, dtype=U64)[:, :self.in_dim])
        d = np.stack(decompose(mask, self.bl, self.L), axis=-1)
        assert np.abs(d).max(initial=0) <= 1 << (self.bl - 1)
        return d.reshape(len(mask), self.in_dim * self.L)

    def __call__(self, cts):
        cts = np.asarray(cts, dtype=U64).reshape(-1, self.in_dim + 1)
        out = np.zeros((len(cts), self.out_size), dtype=U64)
        with np.errstate(over="ignore"):
            for s in range(0, len(cts), 512):                       # bounds the digit matrix, not a tiling of the inputs
                d = self.digits(cts[s:s + 512]).astype(np.float64)
                acc = np.zeros((len(d), self.out_size), dtype=U64)
                for j, limb in enumerate(self.limbs):
                    prod = d @ limb
                    assert np.abs(prod).max(initial=0) <= self.bound
                    acc += prod.astype(np.int64).astype(U64) << U64(LIMB_BITS * j)
                out[s:s + 512] = U64(0) - acc
            out[:, -1] += cts[:, self.in_dim]
        return out


def keyswitch_exact(params, ksk, cts):
    return ExactKeyswitch(params, ksk)(cts)


# ---- edge inputs --------------------------------------------------------------------------------------------------------
#
# Which digit patterns exist.  With B = 2^base_log, a digit of +B/2 is produced only when the raw digit above it is below
# B/2 (iter.rs:113-118: the carry is the top bit of the next raw digit), so two neighbouring levels are never both +B/2,
# and never both -B/2.  "Every digit +B/2" therefore does not exist; the extreme patterns that do are
#     pos      +B/2, B/2 - 1, +B/2, ...   from level 1 down (the largest positive digit sum),
#     neg_max  -B/2, -B/2 + 1, -B/2, ...  from level L up, -B/2 + 1 at level 1 (nothing above it carries: B/2 there stays
#              +B/2) -- the largest negative digit sum; its carry leaves at the top,
#     neg      -B/2 + 1 at every level                      (carry through every level, dropped at the top).
# tests/test_exact_keyswitch.py asserts that the decomposer really yields these digits.
#
# How far this drives the kernels' accumulators (rows at `neg_max` / `pos`, key columns whose eight balanced base-256
# digits are all -128, resp. key words 2^64 - 1 whose eight bytes are all 255):
#   * matrix-core kernel, int32 per (sample, column, plane) and K chunk.  Largest real shape tested, base 7 x 2 levels,
#     k N = 2048, FHESTR_KS_CHUNKS=1 (all 4096 key rows in one workgroup): 2048 * (64 + 63) * 128 = 33 292 288 = 2^24.99,
#     1/64 of 2^31.  PARAM_MESSAGE_2_CARRY_2 (base 3 x 5, one chunk): 2048 * (4 + 3 + 4 + 3 + 4) * 128 = 2^22.2.  The
#     N = 32768 twin with base 7 x 6 levels, two chunks of 4096 steps x 4 elements: 16384 * (3 * 64 + 3 * 63) * 128 =
#     798 916 608 = 2^29.57, 37 % of 2^31 -- the closest any accepted shape comes.
#   * the host's clamp (ks_mfma_max_steps: 32 slots * steps * 2^(base_log + 6) < 2^31) assumes every one of the 32 slots
#     of a step at |digit * key digit| = 2^(base_log + 6).  On the parameter sets of tests/golden/ it never binds (the
#     largest, k N = 32768 with base 3 x 7 levels, has 8192 steps against 131071 allowed).  It CAN bind on accepted shapes:
#     k N = 32768 with base 7 and 6 to 8 levels (8192 steps > 8191) or base 6 and 9 or 10 levels (16384 > 16383); it then
#     forces two chunks where FHESTR_KS_CHUNKS asks for one -- test_gpu_exact_keyswitch.py::test_clamped_chunks runs that
#     case.  By the pattern rule above the true sum stays below 2^31 even unclamped (worst: base 7 x 8 levels,
#     32768 * (4 * 64 + 4 * 63) * 128 = 2^30.99), so the clamp is conservative, never too weak.
#   * byte-plane kernel, u32 per (sample, column, plane) and tile of 64 mask elements: biased digits are at most 2^base_log,
#     key bytes at most 255: 64 * level * 2^base_log * 255 <= 64 * 8 * 128 * 255 = 2^24 for base 7, 64 * 22 * 2 * 255 =
#     2^19.5 for 22 levels of base 1; on the base-7 set tested 64 * 2 * 128 * 255 = 2^22 -- 2^-10 of the u32 range.

def _from_digits(digits_level_L_first, base_log, level):
    """The multiple of 2^(64 - base_log * level) whose digit at level l is digits[level - l], mod 2^64."""
    x = 0
    for it, d in enumerate(digits_level_L_first):
        x += d << (64 - base_log * (level - it))
    return x & M64


def edge_digit_patterns(base_log, level):
    """{name: digits, level L first} of the extreme patterns above."""
    h = 1 << (base_log - 1)
    pos = [h if (level - 1 - it) % 2 == 0 else h - 1 for it in range(level)]            # level 1 (it = level - 1) is +B/2
    neg_max = [-h if it % 2 == 0 and it != level - 1 else -h + 1 for it in range(level)]  # level L (it = 0) is -B/2; level 1 never is
    neg = [-h + 1] * level
    return {"pos": pos, "neg_max": neg_max, "neg": neg}


def edge_mask_values(base_log, level):
    """{name: u64 value} -- the mask elements the issue of this module lists."""
    non_rep = 64 - base_log * level
    mid = 1 << (non_rep - 1)                                    # half a step of the last level: the rounding midpoint
    hi = (0x9E3779B97F4A7C15 >> non_rep) << non_rep             # arbitrary upper digits, nothing below the last level
    v = {"zero": 0, "ones": M64, "mid": mid, "mid_below": mid - 1, "mid_above": (mid + 1) & M64,
         "hi_mid": (hi + mid) & M64, "hi_mid_below": (hi + mid - 1) & M64, "hi_mid_above": (hi + mid + 1) & M64,
         "carry_top": (M64 + 1 - (1 << non_rep)) & M64,         # raw digits all B - 1: digits (-1, 0, ..., 0), carry out of level 1
         "round_wrap": (M64 + 1 - mid) & M64,                   # rounds up to 2^64 = 0
         "below_wrap": (M64 - mid) & M64}                       # one below: stays at 2^64 - 2^non_rep
    for name, digs in edge_digit_patterns(base_log, level).items():
        v[name] = _from_digits(digs, base_log, level)
    v["pos_low"] = (v["pos"] + mid - 1) & M64                  # same digits, the largest value that still rounds to them
    v["neg_max_low"] = (v["neg_max"] - mid) & M64              # same digits, the smallest such value
    return v


N_EDGE_ROWS = 14


def edge_big_cts(params, rng, count):
    """`count` big-key LWEs [count, k N + 1]; the first N_EDGE_ROWS are structured (fewer if count is smaller), the rest
    uniform.  Deterministic given rng.  Rows, in order:
      0 every edge value in turn over the mask, a random word between two of them; body 2^64 - 1
      1 neg_max everywhere; body 0            2 pos everywhere; body 2^63           3 neg everywhere; random body
      4 pos / neg_max alternating by element  5 carry_top everywhere                6 mask 0, body 0   7 mask 2^64 - 1
      8, 9, 10 one non-zero element: the first, the last element of the last complete 16-slot group of the matrix-core
        layout, and k N - 1 (beside the pad slots of the last group)
      11 mid_below / mid / mid_above in turn   12 the same under random upper digits   13 round_wrap / below_wrap / ones"""
    in_dim, bl, L = params.k * params.N, params.ks_base_log, params.ks_level
    v = edge_mask_values(bl, L)
    cts = rng.integers(0, 2**64, size=(count, in_dim + 1), dtype=U64)
    names = list(v)
    idx = np.arange(in_dim)
    rows = []
    r0 = cts[0].copy() if count else None
    if count:
        for j, name in enumerate(names):
            r0[:in_dim][idx % (len(names) + 1) == j] = v[name]
        r0[in_dim] = M64
        rows.append(r0)

    def const(value, body):
        r = np.full(in_dim + 1, value, dtype=U64)
        r[in_dim] = body
        return r

    def cycle(keys, body):
        r = np.zeros(in_dim + 1, dtype=U64)
        for j, key in enumerate(keys):
            r[:in_dim][idx % len(keys) == j] = v[key]
        r[in_dim] = body
        return r

    def single(pos, body):
        r = np.zeros(in_dim + 1, dtype=U64)
        r[pos] = v["neg_max"] if v["neg_max"] else M64
        r[in_dim] = body
        return r

    rand_body = int(rng.integers(0, 2**64, dtype=U64))
    epg = max(1, 16 // L)
    last_full = max(0, in_dim // (2 * epg) * (2 * epg) - 1)
    rows += [const(v["neg_max"], 0), const(v["pos"], 1 << 63), const(v["neg"], rand_body), cycle(["pos", "neg_max"], 1),
             const(v["carry_top"], M64), const(0, 0), const(M64, 1 << 63),
             single(0, 0), single(last_full, 1 << 63), single(in_dim - 1, M64),
             cycle(["mid_below", "mid", "mid_above"], 0), cycle(["hi_mid_below", "hi_mid", "hi_mid_above"], rand_body),
             cycle(["round_wrap", "below_wrap", "ones"], 1 << 63)]
    assert len(rows) == N_EDGE_ROWS or count == 0
    for b, r in enumerate(rows[:count]):
        cts[b] = r
    return cts


def _balanced_word(digits):
    """The u64 whose balanced base-256 digits (least significant first) are `digits`."""
    return sum(d << (8 * t) for t, d in enumerate(digits)) & M64


EDGE_KEY_WORDS = [0, 1, 1 << 63, M64, _balanced_word([-128] * 8), _balanced_word([127] * 8),
                  _balanced_word([-128, 127] * 4), _balanced_word([127, -128] * 4)]


def balanced_digits(word):
    """Eight digits in [-128, 127] with word = sum s_t 256^t (mod 2^64): the rewriting the matrix-core key layout uses."""
    out = []
    for _ in range(8):
        s = ((word & 0xFF) ^ 0x80) - 0x80
        out.append(s)
        word = ((word - s) & M64) >> 8
    return out


def edge_ksk(params, rng):
    """Keyswitch key [k N * level, n + 1], uniform words except: column j < 8 holds EDGE_KEY_WORDS[j] in EVERY row (with the
    pos / neg_max rows of edge_big_cts the whole accumulator column sits at its extreme), columns 8 .. 15 hold them in
    every other row, and the body column n holds the all -128 word in every row (fewer columns: the body column wins)."""
    rows, out_size = params.k * params.N * params.ks_level, params.n + 1
    ksk = rng.integers(0, 2**64, size=(rows, out_size), dtype=U64)
    for j, w in enumerate(EDGE_KEY_WORDS):
        if j < out_size:
            ksk[:, j] = w
        if 8 + j < out_size:
            ksk[j % 2::2, 8 + j] = w
    ksk[:, out_size - 1] = EDGE_KEY_WORDS[4]
    return ksk
