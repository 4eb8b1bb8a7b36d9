"""Cases and references for the integer plans (fhe_int_plan_create), shared by tests/test_integer_sweep_cpu.py and
tests/test_gpu_integer.py.  The references are Python integers; nothing here calls the library.

An unsigned radix integer is n little-endian blocks of `bits` bits.  Every name takes its operands as one flat list of
block messages in the plan's input order: [cond (cmux)], a, [b].  The scalar of a scalar name is a 64-bit unsigned
number: scalar_add and scalar_sub wrap modulo 2^(n bits), the six scalar comparisons compare with the number itself."""
import numpy as np

ARITH = ("add", "sub")
COMPARE = ("eq", "ne", "gt", "ge", "lt", "le")
EXTRACT = ("message_extract", "carry_extract")
TWO_OPERAND = ARITH + COMPARE
SCALAR = tuple("scalar_" + n for n in ARITH + COMPARE)
NAMES = TWO_OPERAND + SCALAR + EXTRACT + ("cmux",)
BOOLEAN = COMPARE + tuple("scalar_" + n for n in COMPARE)
assert len(NAMES) == 19

_CMP = {"eq": lambda a, b: a == b, "ne": lambda a, b: a != b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
        "lt": lambda a, b: a < b, "le": lambda a, b: a <= b}


def to_blocks(value, n, bits):
    return [(value >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def from_blocks(blocks, bits):
    return sum(int(b) << (bits * i) for i, b in enumerate(blocks))


def block_counts(name, bits):
    """1, 2, 3, 4, 5, 8, 9 (the prefix scan has 0, 1, 2, 3 and more steps; odd counts leave the comparator a trailing
    unpacked block), the count that fills 64 bits (the scalar mask edge), and one more where no scalar limits it."""
    full = 64 // bits
    return sorted({1, 2, 3, 4, 5, 8, 9, full} | (set() if name in SCALAR else {full + 1}))


def reference(name, n, bits, inputs, scalar=0):
    """The output block messages of `name` on the flat input messages, from Python integers alone."""
    mod = 1 << (n * bits)
    base = name[7:] if name in SCALAR else name
    if name in EXTRACT:
        m = 1 << bits
        return [(x % m if name == "message_extract" else x // m) for x in inputs]
    if name == "cmux":
        cond, t, f = inputs[0], inputs[1:1 + n], inputs[1 + n:]
        return list(t if cond else f)
    a = from_blocks(inputs[:n], bits)
    b = scalar if name in SCALAR else from_blocks(inputs[n:], bits)          # the scalar unreduced
    if base == "add":
        return to_blocks((a + b) % mod, n, bits)
    if base == "sub":
        return to_blocks((a - b) % mod, n, bits)
    return [int(_CMP[base](a, b))]


def operand_pairs(n, bits, rng, count):
    """`count` pairs (a, b) of n-block integers, at least 40 for the full edge list.  Planted first: 0, 1, 2^w - 1 against each other, equal
    operands, a + b = 2^w - 1 (every block propagates), 2^w - 1 + 1, 0 - 1 (the borrow through every block), neighbours;
    then random pairs, every fourth with equal operands and every fourth adding up to 2^w - 1."""
    w = n * bits
    top = (1 << w) - 1
    rnd = lambda: int.from_bytes(rng.bytes(16), "little") & top
    x = rnd()
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (top, 1), (1, top), (top, top), (top, 0), (0, top), (x, x), (x, top - x), (top - x, x),
             (x, (x + 1) & top), ((x + 1) & top, x), (top >> 1, (top >> 1) + 1 & top), (top >> 1, 1)]
    while len(pairs) < count:
        a, kind = rnd(), len(pairs) % 4
        pairs.append((a, a) if kind == 0 else (a, top - a) if kind == 1 else (a, rnd()))
    return pairs[:max(count, 16)]


def scalar_cases(n, bits, rng, per_scalar=5):
    """[(scalar, [a, ...])]: in-range scalars (0, 1, 2^w - 1, random ones) each met by itself, its neighbours, 0 and 2^w - 1;
    and, where w < 64, the scalars beyond the range: 2^w, 2^w + a, 2^64 - 1."""
    w = n * bits
    top = (1 << w) - 1
    rnd = lambda: int.from_bytes(rng.bytes(16), "little") & top
    cases = []
    for s in [0, 1 & top, top, rnd(), rnd(), top >> 1]:
        ops = [s, (s + 1) & top, (s - 1) & top, 0, top, top - s] + [rnd() for _ in range(max(0, per_scalar - 6))]
        cases.append((s, ops))
    if w < 64:
        a = rnd()
        for s in ((1 << w), (1 << w) + a, (1 << 64) - 1, (1 << w) + top if w < 63 else (1 << 64) - 1):
            cases.append((s, [a, 0, top, 1 & top, rnd(), s & top]))
    return cases


def in_range(scalar, n, bits):
    return scalar >> (n * bits) == 0


def extract_inputs(n, T, M, rng, count):
    """Blocks over the whole box [0, T - 1]: the corners first, then random ones."""
    rows = [[0] * n, [T - 1] * n, [M - 1] * n, [M % T] * n, [(i * (M + 1)) % T for i in range(n)]]
    rows += rng.integers(0, T, size=(max(0, count - len(rows)), n)).tolist()
    return rows


def cmux_inputs(n, bits, rng, count):
    """[cond] + t + f, both conditions for every pair."""
    rows = []
    for a, b in operand_pairs(n, bits, rng, (count + 1) // 2):
        for cond in (0, 1):
            rows.append([cond] + to_blocks(a, n, bits) + to_blocks(b, n, bits))
    return rows


def planted_rows(name, n, bits, T, rng, count, scalar=0):
    """`count` flat input rows for the GPU file: the edge inputs first."""
    M = 1 << bits
    if name in EXTRACT:
        return np.array(extract_inputs(n, T, M, rng, count)[:count], dtype=np.uint64)
    if name == "cmux":
        return np.array(cmux_inputs(n, bits, rng, count)[:count], dtype=np.uint64)
    pairs = operand_pairs(n, bits, rng, count)[:count]
    if name in SCALAR:
        top = (1 << (n * bits)) - 1
        firsts = [scalar & top, (scalar + 1) & top, (scalar - 1) & top]
        return np.array([to_blocks(a, n, bits) for a in (firsts + [p[0] for p in pairs])[:count]], dtype=np.uint64)
    return np.array([to_blocks(a, n, bits) + to_blocks(b, n, bits) for a, b in pairs], dtype=np.uint64)
