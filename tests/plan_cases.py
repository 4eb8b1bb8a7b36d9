"""Random and exhaustive cases for every FheString plan, with their answers from Python `bytes` semantics (as in
scripts/fuzz_strings.py), tests/split_ref.py, tests/count_ref.py and tests/regex_ref.py -- never from the code under test --
and the runner that pushes them through tests/clear_plan.py.  Test infrastructure: tests/test_plan_sweep_cpu.py sweeps
these on the CPU, tests/test_gpu_plan_slots.py draws its device inputs from the same generators.

A Case names one plan (`key`, `build`) and one input (`msgs`, clear block values in the plan's input order), and carries
the reference answer (`want`), the reading of the plan's decoded outputs that is compared with it (`read`), the string
capacity it exercises (`cap`) and the boolean results of the reference by name (`bits`: a sweep must meet both answers of
every one).  Block encodings are restated here (little-endian base-msg_mod digits per character, zero padding); a decoded
string must be left-justified, a bit exactly 0 or 1, a block below msg_mod.

Every generator is seeded by its arguments alone: the same call yields the same cases."""
import itertools
from collections import defaultdict

import numpy as np

from clear_plan import ClearBackend, decode
from count_ref import encode_count, input_digits, repeat_ref, replacen_ref, splitn_ref
from exact_plan import run_ranks
from regex_ref import has_match, random_pattern
from split_ref import ONCE, SPLIT_OPS, decode_split, split_ref

WS = b" \t\n\x0b\x0c\r"
# 15, 16, 17: around one full reduction box at T = 16; 33: two full boxes and one
CAPS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 20, 33)
REGEX_CAPS = (1, 2, 3, 5, 8, 9, 16, 17)
N_MAX = (1, 3, 4, 5, 15, 16)                                  # the digit boundaries of base 4 (and 15 | 16 of base 16)

COMPARE_OPS = ("eq", "ne", "lt", "le", "gt", "ge", "eq_ignore_case", "starts_with", "ends_with", "contains", "find", "rfind")
SAME_CAP = ("eq", "ne", "lt", "le", "gt", "ge", "eq_ignore_case")      # an encrypted right side has the left side's capacity
UNARY_OPS = ("to_upper", "to_lower", "trim_start", "trim_end", "strip", "len", "is_empty")
SHAPE_OPS = UNARY_OPS + ("strip_prefix", "strip_suffix", "concat", "repeat_clear")
FORMS = ("", "_clear", "_reference", "_reference_clear")


class Codec:
    """One parameter set: the library's Params and the block encoding of strings and numbers."""

    def __init__(self, oracle_params):
        from conftest import to_fhestr_params
        self.name = oracle_params.name
        self.P = to_fhestr_params(oracle_params)
        self.M = oracle_params.msg_mod
        self.T = oracle_params.msg_mod * oracle_params.carry_mod
        self.bits = self.M.bit_length() - 1
        self.bpc = 8 // self.bits

    def blocks(self, s: bytes, cap: int):
        assert len(s) <= cap
        return [(ch >> (self.bits * k)) & (self.M - 1) for ch in s.ljust(cap, b"\0") for k in range(self.bpc)]

    def text(self, out):
        assert len(out) % self.bpc == 0 and all(0 <= v < self.M for v in out), ("a string block is a message", out)
        chars = bytes(sum(out[i + k] << (self.bits * k) for k in range(self.bpc)) for i in range(0, len(out), self.bpc))
        assert b"\0" not in chars.rstrip(b"\0"), ("a string is left-justified and zero padded", chars)
        return chars.rstrip(b"\0")

    def number(self, out):
        assert all(0 <= v < self.M for v in out), ("a digit is a message", out)
        return sum(v * self.M ** i for i, v in enumerate(out))

    def digits_for(self, value):
        """How many digits hold 0 .. value."""
        d = 1
        while self.M ** d < value + 1:
            d += 1
        return d

    @staticmethod
    def bit(v):
        assert v in (0, 1), ("a boolean result is 0 or 1", v)
        return v


class Case:
    def __init__(self, label, key, build, msgs, want, read, cap, bits=None):
        self.label, self.key, self.build, self.msgs, self.want, self.read, self.cap = label, key, build, msgs, want, read, cap
        self.bits = bits or {}

    def __repr__(self):
        return f"Case({self.key!r}, msgs={self.msgs!r}, want={self.want!r})"


def op_case(codec, label, name, a_cap, b_cap, clear, operands, want, read, bits=None):
    """A Plan.string_op case; operands: (bytes, capacity) strings and lists of count digits, in input order."""
    msgs = []
    for x in operands:
        msgs += codec.blocks(*x) if isinstance(x, tuple) else list(x)

    def build(P, world):
        import fhestr
        return fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, world, params=P)

    return Case(label, (name, a_cap, b_cap, clear), build, msgs, want, read, a_cap, bits)


def check_noise_bookkeeping(plan, levels, what):
    """The plan's declared worst PBS-input noise, recomputed from what the executor will run: inputs and lookup outputs are
    nominal (variance 1), so a job over DISTINCT sources carries sum_t coeff_t^2 (the definition in csrc/circuit.h).  Every
    job's sources must be distinct, the largest sum must be the declared one, and it must lie within the budget."""
    worst = 0
    for l, lv in enumerate(levels[:-1]):
        if not lv["jobs"]:
            continue
        job = np.repeat(np.arange(lv["jobs"], dtype=np.int64), np.diff(lv["off"].astype(np.int64)))
        pairs = (job << 32) | lv["src"].astype(np.int64)
        assert len(np.unique(pairs)) == len(pairs), f"{what}: a job of level {l} names one source twice"
        nu = np.zeros(lv["jobs"], dtype=np.int64)
        np.add.at(nu, job, lv["coeff"].astype(np.int64) ** 2)
        worst = max(worst, int(nu.max()))
    declared = plan.noise_info()
    assert abs(worst - declared["max_pbs_input_noise"]) < 1e-6, f"{what}: the exported levels reach {worst} nominal variances, the plan declares {declared}"
    assert worst <= declared["budget"] + 1e-9, f"{what}: {worst} nominal variances against a budget of {declared['budget']}"
    return worst


class Sweep:
    """Plans by key (built once, for one world; every one passes check_noise_bookkeeping as it is built) and the check of
    one case: every rank's decoded outputs read as the reference says, no PBS input off a multiple of delta.  A refused
    build is a failure that names the plan."""

    def __init__(self, codec, world=1):
        self.codec, self.world = codec, world
        self.backends, self.share = {}, {}
        self.cases = self.n_pbs = self.padding = self.worst_noise = 0
        self.seen_bits, self.seen_caps = defaultdict(set), set()

    def backend(self, case):
        import fhestr
        be = self.backends.get(case.key)
        if be is None:
            try:
                plan = case.build(self.codec.P, self.world)
            except fhestr.FheError as e:
                raise AssertionError(f"{self.codec.name}: plan build refused: {case.key!r} (world {self.world}): {e}") from None
            be = self.backends[case.key] = ClearBackend(plan, self.codec.P, share=self.share)
            self.worst_noise = max(self.worst_noise, check_noise_bookkeeping(be.plan, be.levels, f"{self.codec.name}: {case.key!r} (world {self.world})"))
        return be

    def outputs(self, case):
        """[decoded outputs of rank r]; the backend keeps the run's bookkeeping."""
        be = self.backend(case)
        be.reset()
        outs, _ = run_ranks(be.plan, case.msgs, be)
        return [decode(self.codec.P, out) for out in outs], be

    def check(self, case):
        outs, be = self.outputs(case)
        for r, out in enumerate(outs):
            got = case.read(out)
            assert got == case.want, f"{self.codec.name} world {self.world} rank {r}: {case!r} gave {got!r} (outputs {out!r})"
        assert be.off_centre == 0, f"{self.codec.name}: {case!r}: {be.off_centre} of {be.n_pbs} PBS inputs are off a multiple of delta"
        self.cases += 1
        self.n_pbs += be.n_pbs
        self.padding += be.padding
        self.seen_caps.add(case.cap)
        for k, v in case.bits.items():
            self.seen_bits[k].add(int(v))

    def assert_coverage(self, caps=CAPS):
        one_sided = {k: v for k, v in self.seen_bits.items() if v != {0, 1}}
        assert not one_sided, f"boolean results that met one answer only: {one_sided}"
        assert self.seen_caps >= set(caps), f"capacities never drawn: {sorted(set(caps) - self.seen_caps)}"


# ---- strings --------------------------------------------------------------------------------------------------------

def all_strings(alphabet: bytes, max_len: int):
    return [bytes(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


def rand_str(rng, alphabet: bytes, max_len: int, min_len: int = 0):
    n = int(rng.integers(min_len, max_len + 1))
    return bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n))


def rand_pattern(rng, alphabet: bytes, a: bytes, cap: int, min_len: int = 0):
    """Often a substring of `a` (positives and overlaps), else a short random one; now and then as long as the capacity, or
    the string and one more character (longer than the string: a near miss)."""
    u = rng.random()
    if len(a) and u < 0.5:
        i = int(rng.integers(0, len(a)))
        b = a[i: int(rng.integers(i + min_len, len(a) + 1))] if i + min_len <= len(a) else a[i:]
    elif u < 0.85:
        b = rand_str(rng, alphabet, min(cap, 4), min_len)
    elif u < 0.93:
        b = rand_str(rng, alphabet, cap, cap)
    else:
        b = a + rand_str(rng, alphabet, 1, 1)
    return b if len(b) >= min_len else rand_str(rng, alphabet, 1, 1)


def padded_cap(rng, b: bytes):
    """The capacity an encrypted pattern is padded to: its length, or one more."""
    return max(1, len(b) + int(rng.integers(0, 2)))


def _seed(codec, *what):
    """A generator seeded by the parameter set's block shape and `what` (names and numbers)."""
    return np.random.default_rng([codec.T, codec.M] + [x for w in what for x in (list(w.encode()) if isinstance(w, str) else [int(w)])])


# ---- family 1: comparisons and searches -------------------------------------------------------------------------------

def compare_ref(op, a, b):
    if op in ("find", "rfind"):
        i = a.find(b) if op == "find" else a.rfind(b)
        return (int(i >= 0), max(i, 0))
    return int({"eq": a == b, "ne": a != b, "lt": a < b, "le": a <= b, "gt": a > b, "ge": a >= b,
                "eq_ignore_case": a.lower() == b.lower(), "starts_with": a.startswith(b), "ends_with": a.endswith(b),
                "contains": b in a}[op])


def compare_case(codec, op, form, a, a_cap, b, b_cap):
    want = compare_ref(op, a, b)
    if op in ("find", "rfind"):
        def read(out):
            assert len(out) == 1 + codec.digits_for(a_cap), (len(out), a_cap)
            found = codec.bit(out[0])
            return (found, codec.number(out[1:]) if found else 0)                 # without a match the index says nothing
        bits = {op: want[0]}
    else:
        def read(out):
            assert len(out) == 1
            return codec.bit(out[0])
        bits = {op: want}
    if form.endswith("_clear"):
        return op_case(codec, op, op + form, a_cap, 0, b, [(a, a_cap)], want, read, bits)
    return op_case(codec, op, op + form, a_cap, b_cap, None, [(a, a_cap), (b, b_cap)], want, read, bits)


def family1_exhaustive(codec, op):
    """All 40 x 40 pairs of strings of length <= 3 over {a, b, B} at capacity 3: the encrypted form on every pair, and one
    of the three other forms, by turns (staggered from row to row)."""
    strings = all_strings(b"abB", 3)
    for i, (a, b) in enumerate(itertools.product(strings, strings)):
        yield compare_case(codec, op, "", a, 3, b, 3)
        yield compare_case(codec, op, FORMS[1 + (i + i // 40) % 3], a, 3, b, 3)


def family1_random(codec, op, count, seed=1):
    rng = _seed(codec, "family1", op, seed)
    alphabet = b"abAB,a \x7f\x01"
    for i in range(count):
        cap = CAPS[i % len(CAPS)] if i < 2 * len(CAPS) else int(rng.choice(CAPS))
        a = rand_str(rng, alphabet, cap)
        b = rand_pattern(rng, alphabet, a, cap)
        form = FORMS[int(rng.integers(0, 4))]
        if form.endswith("_clear"):
            b_cap = 0
        elif op in SAME_CAP:
            b, b_cap = b[:cap], cap
        else:
            b_cap = padded_cap(rng, b)
        yield compare_case(codec, op, form, a, cap, b, b_cap)


# ---- family 2: unary and shape-changing ------------------------------------------------------------------------------

def shape_case(codec, op, form, a, a_cap, b=b"", b_cap=0, n=1):
    """form: "" or "_reference" for the unary operations and repeat_clear (the count n in the clear byte)."""
    text = codec.text
    if op in UNARY_OPS:
        want = {"to_upper": a.upper, "to_lower": a.lower, "trim_start": lambda: a.lstrip(WS), "trim_end": lambda: a.rstrip(WS),
                "strip": lambda: a.strip(WS), "len": lambda: len(a), "is_empty": lambda: int(not a)}[op]()
        read = {"len": codec.number, "is_empty": lambda out: codec.bit(out[0]) if len(out) == 1 else out}.get(op, text)
        return op_case(codec, op, op + form, a_cap, 0, None, [(a, a_cap)], want, read, {op: want} if op == "is_empty" else None)
    if op == "repeat_clear":
        name = "repeat" + form + "_clear"
        return op_case(codec, op, name, a_cap, 0, bytes([n]), [(a, a_cap)], a * n, text)
    if op == "concat":
        want, read, bits = a + b, text, None
    else:
        had = a.startswith(b) if op == "strip_prefix" else a.endswith(b)
        want = (int(had), (a[len(b):] if op == "strip_prefix" else a[:len(a) - len(b)]) if had else a)
        read = lambda out: (codec.bit(out[0]), text(out[1:]))
        bits = {op: had}
    if form.endswith("_clear"):
        return op_case(codec, op, op + form, a_cap, 0, b, [(a, a_cap)], want, read, bits)
    return op_case(codec, op, op + form, a_cap, b_cap, None, [(a, a_cap), (b, b_cap)], want, read, bits)


FAMILY2_PATTERNS = (b"", b"a", b" ", b"A ", b"\na", b"aA", b"a a")


def family2_exhaustive(codec, op):
    """All strings of length <= 4 over {a, A, ' ', newline} at capacities 4 and 5; the two-operand operations meet each
    of them with a pattern of FAMILY2_PATTERNS and a form, both by turns."""
    for cap in (4, 5):
        for i, a in enumerate(all_strings(b"aA \n", 4)):
            if op in UNARY_OPS:
                yield shape_case(codec, op, ("", "_reference")[i % 7 == 0], a, cap)
            elif op == "repeat_clear":
                yield shape_case(codec, op, "", a, cap, n=1 + i % 3)
            else:
                b = FAMILY2_PATTERNS[i % len(FAMILY2_PATTERNS)]
                form = FORMS[(i // len(FAMILY2_PATTERNS)) % 4]
                yield shape_case(codec, op, form, a, cap, b, max(1, len(b) + (i // 28) % 2))


def family2_random(codec, op, count, seed=1):
    rng = _seed(codec, "family2", op, seed)
    alphabet = b"aAbzZ" + WS + b"\x7f\x01@[`{"               # the neighbours of A-Z and a-z among them
    for i in range(count):
        cap = CAPS[i % len(CAPS)] if i < len(CAPS) else int(rng.choice(CAPS))
        a = rand_str(rng, alphabet, cap)
        if rng.random() < 0.4:                                 # whitespace at both ends, and all of it
            a = (rand_str(rng, WS, 3) + a + rand_str(rng, WS, 3))[:cap]
        if op in UNARY_OPS:
            yield shape_case(codec, op, ("", "_reference")[int(rng.random() < 0.2)], a, cap)
        elif op == "repeat_clear":
            yield shape_case(codec, op, "", a, cap, n=int(rng.integers(1, 4)))
        else:
            u = rng.random()
            b = (a[:int(rng.integers(0, len(a) + 1))] if u < 0.35 else a[int(rng.integers(0, len(a) + 1)):] if u < 0.7
                 else rand_pattern(rng, alphabet, a, cap))
            yield shape_case(codec, op, FORMS[int(rng.integers(0, 4))], a, cap, b, padded_cap(rng, b))


# ---- family 3: split and replace -------------------------------------------------------------------------------------

def _ref_form(rng, clear, allowed=True):
    return ("_reference" if rng.random() < 0.15 and allowed else "") + ("_clear" if clear else "")


def split_case(codec, rng, a, cap, b, clear, op=None):
    op = op or str(rng.choice(SPLIT_OPS + ("split_ascii_whitespace",)))
    max_parts = int(rng.integers(1, 6))
    part_cap = int(rng.integers(1, cap + 1)) if rng.random() < 0.4 else None
    tail = ("" if op in ONCE else f":{max_parts}") + (f":{part_cap}" if part_cap is not None else "")
    read = lambda out: decode_split(op, out, codec.M, max_parts, part_cap or cap)
    if op == "split_ascii_whitespace":
        want = split_ref(op, a, None, max_parts, part_cap=part_cap)
        return op_case(codec, op, op + _ref_form(rng, False) + tail, cap, 0, None, [(a, cap)], want, read)
    want = split_ref(op, a, b, max_parts, part_cap=part_cap)
    bits = {op: want[0]} if op in ONCE else None
    name = op + _ref_form(rng, clear) + tail
    if clear:
        return op_case(codec, op, name, cap, 0, b, [(a, cap)], want, read, bits)
    b_cap = padded_cap(rng, b)
    return op_case(codec, op, name, cap, b_cap, None, [(a, cap), (b, b_cap)], want, read, bits)


def _out_cap(rng, full):
    """One below, at or one above the result's length (at least 1)."""
    return max(1, len(full) + int(rng.integers(-1, 2)))


def replace_case(codec, rng, a, cap, b, clear, alphabet):
    """replace (in place, equal lengths), replace:F:C and replacen:n:F:C.  The reference-shaped general replace stops at
    capacity 20: its concatenation tree adds 18 nominal variances per round without looking at the budget, and the six
    rounds of capacity 33 (108) pass the 99.6 of TOY_K1 (PARAM_MESSAGE_2_CARRY_2 holds them: 138.2)."""
    kind = str(rng.choice(["in_place", "general", "general", "replacen", "replacen"]))
    if kind == "in_place":
        b = b[:cap]
        to = rand_str(rng, alphabet, len(b), len(b))
        want = a.replace(b, to)
        form = _ref_form(rng, clear)
        if clear:
            return op_case(codec, "replace", "replace" + form, cap, 0, b + to, [(a, cap)], want, codec.text)
        return op_case(codec, "replace", "replace" + form, cap, 2 * len(b), None, [(a, cap), (b, len(b)), (to, len(b))], want, codec.text)
    to = rand_str(rng, alphabet, 3)
    n = int(rng.integers(0, 4)) if kind == "replacen" else None
    full = a.replace(b, to) if n is None else a.replace(b, to, n)
    out_cap = _out_cap(rng, full)
    base, lead = ("replace", "") if n is None else ("replacen", f":{n}")
    form = _ref_form(rng, clear, cap <= 20)
    if clear:
        return op_case(codec, base, f"{base}{form}{lead}:{len(b)}:{out_cap}", cap, 0, b + to, [(a, cap)], full[:out_cap], codec.text)
    f_cap, t_cap = padded_cap(rng, b), padded_cap(rng, to)
    return op_case(codec, base, f"{base}{form}{lead}:{f_cap}:{out_cap}", cap, f_cap + t_cap, None,
                   [(a, cap), (b, f_cap), (to, t_cap)], full[:out_cap], codec.text)


def family3(codec, count, seed=1):
    rng = _seed(codec, "family3", seed)
    for i in range(count):
        cap = CAPS[i % len(CAPS)] if i < 2 * len(CAPS) else int(rng.choice(CAPS))
        whitespace = rng.random() < 0.12
        alphabet = b"ab" + WS if whitespace else b"ab,a "
        a = rand_str(rng, alphabet, cap)
        b = rand_pattern(rng, alphabet, a, cap, min_len=1)       # a clear empty separator is refused, an encrypted one separates nothing
        clear = bool(rng.random() < 0.5)
        if whitespace:
            yield split_case(codec, rng, a, cap, b, clear, op="split_ascii_whitespace")
        elif rng.random() < 0.55:
            yield split_case(codec, rng, a, cap, b, clear, op=str(rng.choice(SPLIT_OPS)))
        else:
            yield replace_case(codec, rng, a, cap, b, clear, alphabet)


# ---- family 4: encrypted counts --------------------------------------------------------------------------------------

def family4(codec, count, seed=1):
    """repeat:M, replacen_encn[_clear], splitn_encn[_clear], rsplitn_encn[_clear]: n_max over N_MAX, n from 0 to whatever
    the digits of n_max hold (n > n_max acts as n_max).  repeat's result has n_max * cap characters: its capacities stop
    where that passes 80."""
    rng = _seed(codec, "family4", seed)
    alphabet = b"ab,a "
    M = codec.M
    for i in range(count):
        cap = CAPS[i % len(CAPS)] if i < 2 * len(CAPS) else int(rng.choice(CAPS))
        kind = ("repeat", "replacen", "splitn", "rsplitn")[int(rng.integers(0, 4))]
        n_max = int(rng.choice([m for m in N_MAX if kind != "repeat" or m * cap <= 80]))
        held = M ** input_digits(M, n_max) - 1
        n = int(rng.choice([0, n_max, min(n_max + 1, held), held, int(rng.integers(0, held + 1))]))
        digits = encode_count(M, n, n_max)
        a = rand_str(rng, alphabet, cap)
        b = rand_pattern(rng, alphabet, a, cap, min_len=1)
        clear = bool(rng.random() < 0.5)
        if kind == "repeat":
            yield op_case(codec, "repeat", f"repeat:{n_max}", cap, 0, None, [(a, cap), digits], repeat_ref(a, n, n_max), codec.text)
        elif kind == "replacen":
            to = rand_str(rng, alphabet, 3)
            full = replacen_ref(a, b, to, n, n_max)
            out_cap = _out_cap(rng, full)
            if clear:
                yield op_case(codec, "replacen_encn", f"replacen_encn_clear:{n_max}:{len(b)}:{out_cap}", cap, 0, b + to,
                              [(a, cap), digits], full[:out_cap], codec.text)
            else:
                f_cap, t_cap = padded_cap(rng, b), padded_cap(rng, to)
                yield op_case(codec, "replacen_encn", f"replacen_encn:{n_max}:{f_cap}:{out_cap}", cap, f_cap + t_cap, None,
                              [(a, cap), (b, f_cap), (to, t_cap), digits], full[:out_cap], codec.text)
        else:
            part_cap = int(rng.integers(1, cap + 1)) if rng.random() < 0.4 else None
            name = f"{kind}_encn" + ("_clear" if clear else "") + f":{n_max}" + (f":{part_cap}" if part_cap is not None else "")
            want = splitn_ref(kind, a, b, n, n_max, part_cap=part_cap)
            read = lambda out, n_max=n_max, pc=part_cap or cap: decode_split("splitn", out, M, n_max, pc)
            if clear:
                yield op_case(codec, kind + "_encn", name, cap, 0, b, [(a, cap), digits], want, read)
            else:
                b_cap = padded_cap(rng, b)
                yield op_case(codec, kind + "_encn", name, cap, b_cap, None, [(a, cap), (b, b_cap), digits], want, read)


# ---- family 5: matches_clear -----------------------------------------------------------------------------------------

def regex_strings(rng, cap, count=6):
    for _ in range(count):
        n = int(rng.integers(0, cap + 1))
        yield bytes(rng.choice(list(b"abcB.\n"), size=n, p=[.3, .3, .25, .05, .05, .05]).tolist())


def family5(codec, patterns, seed=1):
    rng = _seed(codec, "family5", seed)
    for i in range(patterns):
        pattern = random_pattern(rng, int(rng.integers(1, 9)))
        cap = REGEX_CAPS[i % len(REGEX_CAPS)] if i < len(REGEX_CAPS) else int(rng.choice(REGEX_CAPS))
        for s in regex_strings(rng, cap):
            want = has_match(s, pattern)
            yield op_case(codec, "matches", "matches_clear", cap, 0, pattern, [(s, cap)], want,
                          lambda out: codec.bit(out[0]) if len(out) == 1 else out, {"matches": want})


# ---- family 6: string programs ---------------------------------------------------------------------------------------

PROGRAM_CAPS = (2, 3, 5, 8)
PROGRAM_FINALS = ("str", "len", "eq", "contains", "find")


def _program_steps(b, to):
    """(name, apply(program, value, w) -> value, reference(string, w) -> string): string-to-string steps; `w` is the
    program's second input, which some steps take as their (encrypted, zero padded) pattern."""
    cut = lambda s, p: s[len(p):] if s.startswith(p) else s
    cut_end = lambda s, p: s[:len(s) - len(p)] if s.endswith(p) else s
    return [
        ("to_upper", lambda p, v, w: p.to_upper(v), lambda s, t: s.upper()),
        ("to_lower", lambda p, v, w: p.to_lower(v), lambda s, t: s.lower()),
        ("strip", lambda p, v, w: p.strip(v), lambda s, t: s.strip(WS)),
        ("trim_start", lambda p, v, w: p.trim_start(v), lambda s, t: s.lstrip(WS)),
        ("trim_end", lambda p, v, w: p.trim_end(v), lambda s, t: s.rstrip(WS)),
        ("strip_prefix", lambda p, v, w: p.strip_prefix(v, b)[1], lambda s, t: cut(s, b)),
        ("strip_prefix_w", lambda p, v, w: p.strip_prefix(v, w)[1], lambda s, t: cut(s, t)),
        ("strip_suffix", lambda p, v, w: p.strip_suffix(v, b)[1], lambda s, t: cut_end(s, b)),
        ("concat", lambda p, v, w: p.concat(v, b), lambda s, t: s + b),
        ("concat_w", lambda p, v, w: p.concat(v, w), lambda s, t: s + t),
        ("replace", lambda p, v, w: p.replace(v, b, to, out_cap=v.cap + 2), lambda s, t: s.replace(b, to)),
        ("split_once_1", lambda p, v, w: p.split_once(v, b).parts[1], lambda s, t: s.partition(b)[2]),
        ("rsplit_0", lambda p, v, w: p.rsplit(v, b, 2).parts[0], lambda s, t: s.rsplit(b)[-1]),
    ]


class ProgramShape:
    """One random chain of 2 to 4 steps on the first input, ended by one of PROGRAM_FINALS; the second input `w` feeds
    the end (eq, contains) and, for the `_w` steps, the chain as well: then it is consumed twice."""

    def __init__(self, rng, index):
        alphabet = b"abAB ,a"
        self.cap = PROGRAM_CAPS[index % len(PROGRAM_CAPS)]
        self.b = rand_str(rng, alphabet, 2, 1)
        self.to = rand_str(rng, alphabet, 3)
        table = _program_steps(self.b, self.to)
        self.steps = [table[int(i)] for i in rng.integers(0, len(table), size=int(rng.integers(2, 5)))]
        self.final = PROGRAM_FINALS[int(rng.integers(0, len(PROGRAM_FINALS)))]
        self.dedupe = bool(rng.integers(0, 2))
        self.key = ("program", self.cap, self.b, self.to, tuple(s[0] for s in self.steps), self.final, self.dedupe)
        self.w_uses = sum(s[0].endswith("_w") for s in self.steps) + (self.final in ("eq", "contains"))    # (eq: if the capacities agree)
        self.caps = None                       # [capacity after step i], known once the program is built

    def record(self, params, engine=None):
        """The StringProgram, not compiled."""
        import fhestr
        prog = fhestr.StringProgram(engine, params=params, dedupe=self.dedupe)
        v, w = prog.string(self.cap), prog.string(self.cap)
        self.caps = []
        for _, apply, _ in self.steps:
            v = apply(prog, v, w)
            self.caps.append(v.cap)
        if self.final == "str":
            prog.output(v)
        elif self.final == "len":
            prog.output(prog.len(v))
        elif self.final == "eq":
            prog.output(prog.eq(prog.to_lower(v), prog.to_lower(w)) if v.cap == w.cap else prog.eq_ignore_case(v, self.b))
        elif self.final == "contains":
            prog.output(prog.contains(v, w))
        else:
            prog.output(*prog.find(v, self.b))
        return prog

    def build(self, P, world):
        return self.record(P).compile(world).plan

    def reference(self, s, t):
        """(want, cut): cut = an intermediate result did not fit its capacity (the case is then left out)."""
        r, cut = s, False
        for (_, _, ref), cap in zip(self.steps, self.caps):
            r = ref(r, t)
            cut = cut or len(r) > cap
        if self.final == "str":
            return r, cut
        if self.final == "len":
            return len(r), cut
        if self.final == "eq":
            return int(r.lower() == (t if self.caps[-1] == self.cap else self.b).lower()), cut
        if self.final == "contains":
            return int(t in r), cut
        i = r.find(self.b)
        return (int(i >= 0), max(i, 0)), cut

    def case(self, codec, s, t):
        want, cut = self.reference(s, t)
        read = {"str": codec.text, "len": codec.number, "eq": lambda out: codec.bit(out[0]) if len(out) == 1 else out,
                "contains": lambda out: codec.bit(out[0]) if len(out) == 1 else out,
                "find": lambda out: (codec.bit(out[0]), codec.number(out[1:]) if out[0] else 0)}[self.final]
        bits = {} if self.final in ("str", "len") else {"program " + self.final: want[0] if self.final == "find" else want}
        msgs = codec.blocks(s, self.cap) + codec.blocks(t, self.cap)
        return Case("program", self.key, self.build, msgs, want, read, self.cap, bits), cut


def family6(codec, programs, inputs_each=4, seed=1):
    """(case, cut) pairs: `programs` random chains, `inputs_each` inputs for each.  The shape's capacities are known only
    once its program has been recorded, which the first reference() needs: record() runs here, offline."""
    rng = _seed(codec, "family6", seed)
    alphabet = b"abAB ,a"
    for i in range(programs):
        shape = ProgramShape(rng, i)
        shape.record(codec.P).close()
        for _ in range(inputs_each):
            s = rand_str(rng, alphabet, shape.cap)
            u = rng.random()
            t = rand_str(rng, alphabet, shape.cap) if u < 0.4 else s[int(rng.integers(0, len(s) + 1)):] if u < 0.7 else s[:int(rng.integers(0, len(s) + 1))]
            yield shape.case(codec, s, t)


# ---- named plans for the tests that compare executors (tests/test_clear_plan.py, tests/test_gpu_plan_slots.py) ---------

def three_step_program(params, engine=None, world=1):
    """to_lower, strip, then the part behind the first comma: three chained operations on one string of capacity 8, one
    plan.  Returns the compiled program; its reference is three_step_reference."""
    import fhestr
    prog = fhestr.StringProgram(engine, params=params)
    a = prog.string(8)
    prog.output(prog.split_once(prog.strip(prog.to_lower(a)), b",").parts[1])
    return prog.compile(world)


def three_step_reference(s: bytes) -> bytes:
    return s.lower().strip(WS).partition(b",")[2]
