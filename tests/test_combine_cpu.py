"""Combining results -- bit logic, select, arithmetic and comparisons on counts -- without a GPU: the C++ planner builds
offline plans on TOY_K1 (msg_mod = 4, a box of 16), the CPU oracle executes their exported levels, and what decrypts is
compared with the clear-text definitions of tests/combine_ref.py.

Counts travel in base-4 digits: bounds up to 3 are one digit, up to 15 two (one packed unit), 16 takes three, so the
bounds 5 / 4 cross a digit boundary inside one unit and 16 / 16 runs the radix code with its clamp."""
import itertools

import numpy as np
import pytest

import oracle as O
from combine_ref import (COMPARISONS, COUNT_OPS, bits_ref, clear_bytes, count_bound, count_ref, decode_bit, decode_digits, decode_string,
                         select_count_ref, select_ref)
from conftest import to_fhestr_params
from count_ref import encode_count, input_digits
from plan_oracle import run_with_oracle
from test_count_cpu import _run_two_ranks

M = O.TOY_K1.msg_mod
BPC = 4
A_CAP = 8


def _params(p=O.TOY_K1):
    return to_fhestr_params(p)


_PLANS = {}


def _plan(op, a_cap=0, b_cap=0, clear=None, world=1, params=None):
    import fhestr
    key = (op, a_cap, b_cap, clear, world, (params or O.TOY_K1).name)
    if key not in _PLANS:
        _PLANS[key] = fhestr.Plan.string_op(None, op, a_cap, b_cap, clear, world, params=_params(params or O.TOY_K1))
        noise = _PLANS[key].noise_info()
        assert noise["max_pbs_input_noise"] <= noise["budget"], key
    return _PLANS[key]


def _enc(ks, s, cap):
    import fhestr
    return ks.ck.encrypt_many(fhestr.string_to_blocks(_params(), s, cap))


def _enc_count(ks, n, n_max):
    return ks.ck.encrypt_many(np.array(encode_count(M, n, n_max), dtype=np.uint64))


def _enc_bit(ks, b):
    return ks.ck.encrypt_many(np.array([b], dtype=np.uint64))


def _run(ks, plan, operands, run=run_with_oracle):
    """The raw outputs (ciphertexts) of one run on the operands in plan order."""
    inputs = np.concatenate(operands)
    assert plan.info()["n_inputs"] == len(inputs)
    return run(plan, inputs, ks.sk)


def _msgs(ks, cts):
    return [int(m) for m in np.asarray(ks.ck.decrypt_many(cts)).reshape(-1)]


# ---- bit logic ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ("and", "or", "xor"))
@pytest.mark.parametrize("k", (2, 3))
def test_truth_tables(toy_k1, op, k):
    plan = _plan(f"{op}:{k}")
    for bits in itertools.product((0, 1), repeat=k):
        got = decode_bit(_msgs(toy_k1, _run(toy_k1, plan, [_enc_bit(toy_k1, b) for b in bits])))
        assert got == bits_ref(op, bits), (op, bits, got)


@pytest.mark.parametrize("op", ("and", "or", "xor"))
def test_more_bits_than_one_lookup_holds(toy_k1, op):
    """k = 17: one more than the 16 bits a full-box lookup sums, so the reduction has two levels."""
    k = O.TOY_K1.msg_mod * O.TOY_K1.carry_mod + 1
    plan = _plan(f"{op}:{k}")
    assert plan.info()["n_levels"] == 2
    cases = [[1] * k, [0] * k, [0] + [1] * (k - 1), [1] * (k - 1) + [0], [0] * (k - 1) + [1], [1] + [0] * (k - 1), [1, 0] * (k // 2) + [1]]
    for bits in cases:
        got = decode_bit(_msgs(toy_k1, _run(toy_k1, plan, [_enc_bit(toy_k1, b) for b in bits])))
        assert got == bits_ref(op, bits), (op, bits, got)


@pytest.mark.parametrize("k", (1, 3))
def test_not(toy_k1, k):
    plan = _plan(f"not:{k}")
    for bits in itertools.product((0, 1), repeat=k):
        got = _msgs(toy_k1, _run(toy_k1, plan, [_enc_bit(toy_k1, b) for b in bits]))
        assert got == bits_ref("not", bits), (bits, got)


# ---- select ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", (4, 5, 7), ids=("cut", "exact", "padded"))
def test_select_strings_of_unequal_capacity(toy_k1, cap):
    """a in 5 characters, b in 3: C = 4 cuts a, C = 5 fits it, C = 7 pads both; an empty side; both values of the bit."""
    plan = _plan(f"select:{cap}", 5, 3)
    assert plan.info()["n_outputs"] == cap * BPC
    for a, b in ((b"abcde", b"xyz"), (b"ab", b"x"), (b"", b"xyz"), (b"abcde", b""), (b"", b"")):
        for c in (0, 1):
            out = _run(toy_k1, plan, [_enc(toy_k1, a, 5), _enc(toy_k1, b, 3), _enc_bit(toy_k1, c)])
            assert decode_string(_msgs(toy_k1, out), M, cap) == select_ref(c, a, b, cap), (a, b, c, cap)
    assert select_ref(1, b"abcde", b"xyz", 4) == b"abcd" and select_ref(0, b"abcde", b"xyz", 7) == b"xyz"


@pytest.mark.parametrize("cap", (4, 5, 7))
def test_select_clear(toy_k1, cap):
    for b in (b"xyz", b"", b"xyzuvwxy"):
        plan = _plan(f"select_clear:{cap}", 5, 0, b)
        for a in (b"abcde", b"ab", b""):
            for c in (0, 1):
                out = _run(toy_k1, plan, [_enc(toy_k1, a, 5), _enc_bit(toy_k1, c)])
                assert decode_string(_msgs(toy_k1, out), M, cap) == select_ref(c, a, b, cap), (a, b, c, cap)


@pytest.mark.parametrize("a_max,b_max", ((3, 16), (16, 3), (3, 3)))
def test_select_count_bounds_that_differ_in_digits(toy_k1, a_max, b_max):
    assert (input_digits(M, 3), input_digits(M, 16)) == (1, 3)
    plan = _plan(f"select_count:{a_max}:{b_max}")
    for a, b in ((0, 0), (a_max, b_max), (1, b_max - 1), (a_max - 1, 2)):
        for c in (0, 1):
            out = _run(toy_k1, plan, [_enc_count(toy_k1, a, a_max), _enc_count(toy_k1, b, b_max), _enc_bit(toy_k1, c)])
            assert decode_digits(_msgs(toy_k1, out), M, max(a_max, b_max)) == select_count_ref(c, a, b), (a, b, c)


# ---- count arithmetic -----------------------------------------------------------------------------------------------------------

def _count(ks, op, a, a_max, b, b_max=None, run=run_with_oracle, world=1):
    """The decoded result of count_<op>; b_max=None: b is the clear integer."""
    if b_max is None:
        plan = _plan(f"count_{op}_clear:{a_max}", clear=clear_bytes(b), world=world)
        operands = [_enc_count(ks, a, a_max)]
    else:
        plan = _plan(f"count_{op}:{a_max}:{b_max}", world=world)
        operands = [_enc_count(ks, a, a_max), _enc_count(ks, b, b_max)]
    msgs = _msgs(ks, _run(ks, plan, operands, run))
    if op in COMPARISONS:
        return decode_bit(msgs)
    return decode_digits(msgs, M, count_bound(op, a_max, b if b_max is None else b_max))


@pytest.mark.parametrize("op", COUNT_OPS)
def test_every_pair_across_a_digit_boundary(toy_k1, op):
    """a_max = 5, b_max = 4: two digits each, one packed unit; every pair within the bounds, and operands above their
    bound, which act as the bound."""
    assert count_ref("add", 5, 5, 4, 4) == 9 and count_ref("sub", 2, 5, 4, 4) == 0 and count_ref("sub", 15, 5, 15, 4) == 1
    for a, b in list(itertools.product(range(6), range(5))) + [(6, 0), (15, 4), (3, 5), (5, 15), (15, 15), (9, 7)]:
        got = _count(toy_k1, op, a, 5, b, 4)
        assert got == count_ref(op, a, 5, b, 4), (op, a, b, got)


# the carry points 3+1, 15+1 and 16+16, the borrow points 4-1, 16-1, 0-1 and 2-5, the pairs beside them, and operands above 16
PAIRS_16 = [(3, 1), (3, 0), (2, 1), (4, 1), (15, 1), (15, 0), (14, 1), (16, 1), (16, 16), (16, 15), (15, 16), (15, 15),
            (4, 0), (5, 1), (16, 0), (16, 2), (0, 1), (0, 0), (1, 1), (1, 2), (2, 5), (2, 4), (3, 5), (5, 2), (2, 2), (12, 12), (11, 5),
            (17, 3), (63, 63), (20, 16), (7, 31)]


@pytest.mark.parametrize("op", COUNT_OPS)
def test_three_digits_at_the_carry_and_borrow_points(toy_k1, op):
    assert input_digits(M, 16) == 3
    for a, b in PAIRS_16:
        got = _count(toy_k1, op, a, 16, b, 16)
        assert got == count_ref(op, a, 16, b, 16), (op, a, b, got)


BESIDE = [   # (a_max, b_max, a values, b values): the sums whose clamps run beside the carry chain
    (16, 5, (0, 1, 3, 4, 11, 12, 15, 16, 17, 31, 48, 63), tuple(range(16))),
    (8, 32, tuple(range(16)), (0, 1, 7, 8, 15, 16, 24, 31, 32, 33, 63)),
    (2, 16, (0, 1, 2, 3), (0, 1, 2, 13, 14, 15, 16, 17, 63)),
    (32, 32, (0, 1, 15, 16, 17, 31, 32, 33, 47, 63), (0, 1, 15, 16, 17, 31, 32, 48, 63)),
    (48, 63, (0, 15, 16, 47, 48, 49, 63), (0, 1, 15, 16, 17, 48, 63)),
]


@pytest.mark.parametrize("a_max,b_max,values_a,values_b", BESIDE, ids=[f"{c[0]}-{c[1]}" for c in BESIDE])
def test_count_add_with_the_clamps_beside_the_carry_chain(toy_k1, a_max, b_max, values_a, values_b):
    """Three-digit bounds that are multiples of 16 or fill their digits, and a second operand of one unit with any bound: every
    carry point of the low unit and of digit 0, with neither, one and both operands above their bound."""
    for a, b in itertools.product(values_a, values_b):
        got = _count(toy_k1, "add", a, a_max, b, b_max)
        assert got == count_ref("add", a, a_max, b, b_max), (a_max, b_max, a, b, got)


@pytest.mark.parametrize("op", COUNT_OPS)
def test_single_digits_and_unequal_digit_counts(toy_k1, op):
    """3 / 3: two single digits, one bivariate lookup; 2 / 2: the digits hold more than the bound; 3 / 16 and 40 / 5: operands
    of different lengths in the radix code."""
    for a_max, b_max, pairs in ((3, 3, itertools.product(range(4), repeat=2)), (2, 2, ((0, 0), (2, 2), (3, 1), (1, 3), (3, 3), (2, 1))),
                                (3, 16, ((3, 16), (0, 16), (3, 0), (2, 3), (3, 2), (3, 63), (1, 1))),
                                (40, 5, ((40, 5), (39, 5), (3, 5), (5, 5), (4, 5), (16, 1), (15, 1), (63, 15), (0, 0)))):
        for a, b in pairs:
            got = _count(toy_k1, op, a, a_max, b, b_max)
            assert got == count_ref(op, a, a_max, b, b_max), (op, a_max, b_max, a, b, got)


@pytest.mark.parametrize("op", COUNT_OPS)
def test_clear_second_operand_of_one_and_two_bytes(toy_k1, op):
    """a_max = 8: one unit, every digit one lookup; 16: the radix code's scalar forms; 300 with the integer 261: two bytes."""
    assert len(clear_bytes(5)) == 1 and clear_bytes(261) == b"\x05\x01"
    for a_max, ks, values in ((8, (0, 1, 5, 8, 9, 200), (0, 1, 4, 5, 7, 8, 9, 15)), (16, (0, 1, 5, 16, 17), (0, 1, 3, 4, 5, 15, 16, 17, 63)),
                              (300, (261,), (0, 39, 260, 261, 262, 300, 1023))):
        for k in ks:
            for a in values:
                got = _count(toy_k1, op, a, a_max, k)
                assert got == count_ref(op, a, a_max, k), (op, a_max, a, k, got)


# ---- results as operands, no glue -----------------------------------------------------------------------------------------------

def test_len_plus_a_clear_integer_feeds_skip(toy_k1):
    """len (n_max = 8) -> count_add_clear:8 with 1 (n_max = 9) -> skip_encn:9, and -> count_sub_clear:8 with 2 -> take_encn:8: the
    output ciphertexts of one plan are the inputs of the next as they are."""
    for s in (b"abcdefgh", b"abcde", b"ab", b"a", b""):
        digits = _run(toy_k1, _plan("len", A_CAP), [_enc(toy_k1, s, A_CAP)])
        plus = _run(toy_k1, _plan("count_add_clear:8", clear=b"\x01"), [digits])
        assert decode_digits(_msgs(toy_k1, plus), M, 9) == len(s) + 1
        rest = _run(toy_k1, _plan("skip_encn:9", A_CAP), [_enc(toy_k1, s, A_CAP), plus])
        assert decode_string(_msgs(toy_k1, rest), M, A_CAP) == s[len(s) + 1:] == b""
        minus = _run(toy_k1, _plan("count_sub_clear:8", clear=b"\x02"), [digits])
        head = _run(toy_k1, _plan("take_encn:8", A_CAP), [_enc(toy_k1, s, A_CAP), minus])
        assert decode_string(_msgs(toy_k1, head), M, A_CAP) == s[:max(len(s) - 2, 0)], s


def test_the_value_after_the_separator(toy_k1):
    """s[find(s, ":") + 1:] = s.split(b":", 1)[1] where the separator is found."""
    for s in (b"key:val", b":abc", b"abcdefg:", b"a:b:c", b"k:", b"colour:b"):
        out = _run(toy_k1, _plan("find_clear", A_CAP, 0, b":"), [_enc(toy_k1, s, A_CAP)])
        assert decode_bit(_msgs(toy_k1, out[:1])) == 1
        plus = _run(toy_k1, _plan("count_add_clear:8", clear=b"\x01"), [out[1:]])
        rest = _run(toy_k1, _plan("skip_encn:9", A_CAP), [_enc(toy_k1, s, A_CAP), plus])
        assert decode_string(_msgs(toy_k1, rest), M, A_CAP) == s.split(b":", 1)[1], s


# ---- programs -------------------------------------------------------------------------------------------------------------------

def _program():
    import fhestr
    return fhestr.StringProgram(None, params=_params())


def _run_program(ks, compiled, inputs, run=run_with_oracle):
    import fhestr
    msgs = ks.ck.decrypt_many(run(compiled.plan, np.concatenate(inputs), ks.sk)).reshape(-1, 1)
    out = []
    for x in compiled.results_of(msgs):
        if isinstance(x, fhestr.EncryptedCount):
            out.append(decode_digits(np.asarray(x.digits).reshape(-1), M, x.n_max))
        elif np.asarray(x).size == 1:
            out.append(decode_bit(np.asarray(x).reshape(-1)))
        else:
            out.append(fhestr.blocks_to_string(_params(), x))
    return tuple(out)


TEXTS = (b"abcxdefb", b"axb", b"abc", b"xyz", b"b", b"", b"aXb", b"a", b"xxxxxxxx")


def test_program_upper_case_if_it_contains_x(toy_k1):
    prog = _program()
    s = prog.string(A_CAP)
    out = prog.select(prog.contains(s, b"x"), prog.to_upper(s), s)
    assert (out.kind, out.cap) == ("string", A_CAP)
    prog.output(out)
    compiled = prog.compile()
    assert sum(b"x" in t for t in TEXTS) >= 3 and sum(b"x" not in t for t in TEXTS) >= 3
    for t in TEXTS:
        assert _run_program(toy_k1, compiled, [_enc(toy_k1, t, A_CAP)]) == (t.upper() if b"x" in t else t,), t


def _affix_program(negate):
    prog = _program()
    s = prog.string(A_CAP)
    ends = prog.ends_with(s, b"b")
    prog.output(prog.bit_and(prog.starts_with(s, b"a"), prog.bit_not(ends) if negate else ends))
    return prog.compile()


def test_program_starts_with_a_and_does_not_end_with_b(toy_k1):
    compiled = _affix_program(True)
    want = [int(t.startswith(b"a") and not t.endswith(b"b")) for t in TEXTS]
    assert sum(want) >= 2 and len(want) - sum(want) >= 4
    for t, w in zip(TEXTS, want):
        assert _run_program(toy_k1, compiled, [_enc(toy_k1, t, A_CAP)]) == (w,), t


def test_program_not_adds_no_lookup():
    with_not, without = _affix_program(True).plan.info(), _affix_program(False).plan.info()
    assert (with_not["n_pbs"], with_not["n_levels"]) == (without["n_pbs"], without["n_levels"])
    # ... also where the negation is an output
    prog = _program()
    s = prog.string(4)
    base = prog.is_empty(s)
    n_before = prog.n_ops
    prog.output(prog.bit_not(base))
    assert prog.n_ops == n_before + 1
    alone = _program()
    alone.output(alone.is_empty(alone.string(4)))
    assert prog.compile().plan.info()["n_pbs"] == alone.compile().plan.info()["n_pbs"]


PAIRS = ((b"abc", b"xy"), (b"ab", b"xyz"), (b"", b"x"), (b"abcde", b""), (b"ab", b"xy"), (b"abcde", b"xyz"), (b"a", b"xyz"), (b"", b""))


def _shorter_program(world=1):
    prog = _program()
    a, b = prog.string(5), prog.string(3)
    la, lb = prog.len(a), prog.len(b)
    lt = prog.count_lt(la, lb)
    assert (lt.kind, la.n_max, lb.n_max) == ("bit", 5, 3)
    shorter = prog.select(lt, a, b)
    assert shorter.cap == 5
    prog.output(shorter, prog.count_min(la, lb), prog.select(lt, la, lb), prog.count_max(la, lb), prog.count_add(la, lb), prog.count_sub(la, lb))
    return prog.compile(world)


def test_program_the_shorter_string_and_count_min(toy_k1):
    """select(count_lt(len(a), len(b)), a, b); count_min is that comparison and a select_count (the same values, and with
    deduplication the same nodes: it adds no lookup)."""
    compiled = _shorter_program()
    assert sum(len(a) < len(b) for a, b in PAIRS) >= 3 and sum(len(a) >= len(b) for a, b in PAIRS) >= 3
    for a, b in PAIRS:
        got = _run_program(toy_k1, compiled, [_enc(toy_k1, a, 5), _enc(toy_k1, b, 3)])
        lo, hi = min(len(a), len(b)), max(len(a), len(b))
        assert got == (a if len(a) < len(b) else b, lo, lo, hi, len(a) + len(b), max(len(a) - len(b), 0)), (a, b, got)
    prog = _program()
    a, b = prog.string(5), prog.string(3)
    la, lb = prog.len(a), prog.len(b)
    prog.output(prog.select(prog.count_lt(la, lb), la, lb))
    by_hand = prog.compile().plan.info()["n_pbs"]
    prog = _program()
    a, b = prog.string(5), prog.string(3)
    m = prog.count_min(prog.len(a), prog.len(b))
    assert (m.kind, m.n_max) == ("count", 5)
    prog.output(m)
    assert prog.compile().plan.info()["n_pbs"] == by_hand


def test_program_built_for_two_ranks(toy_k1):
    compiled = _shorter_program(world=2)
    assert compiled.plan.info()["world"] == 2
    for a, b in PAIRS[:4]:
        got = _run_program(toy_k1, compiled, [_enc(toy_k1, a, 5), _enc(toy_k1, b, 3)], run=_run_two_ranks)
        assert got[0] == (a if len(a) < len(b) else b) and got[1] == min(len(a), len(b)), (a, b, got)


def test_program_bit_input_and_count_input(toy_k1):
    """A bit input chooses between a string and clear bytes; count inputs feed min / max with an int."""
    prog = _program()
    c, s, n = prog.bit(), prog.string(4), prog.count(9)
    assert (c.kind, c.blocks) == ("bit", 1)
    prog.output(prog.select(c, s, b"no"), prog.bit_xor(c, prog.is_empty(s)), prog.count_min(n, 4), prog.count_max(n, 4), prog.count_ge(n, 4))
    compiled = prog.compile()
    for bit, text, k in ((1, b"yes", 0), (0, b"yes", 3), (1, b"", 4), (0, b"", 5), (1, b"abcd", 9), (0, b"abcd", 15)):
        got = _run_program(toy_k1, compiled, [_enc_bit(toy_k1, bit), _enc(toy_k1, text, 4), _enc_count(toy_k1, k, 9)])
        kk = min(k, 9)
        assert got == (text if bit else b"no", bit ^ int(not text), min(kk, 4), max(kk, 4), int(kk >= 4)), (bit, text, k, got)


# ---- conditions, from Plan.info() -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", (O.TOY_K1, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS), ids=lambda p: p.name)
def test_lookup_and_level_counts(params):
    for op in ("and:2", "or:2", "xor:2"):
        info = _plan(op, params=params).info()
        assert (info["n_pbs"], info["n_levels"]) == (1, 1), op
    for a_cap, b_cap, cap in ((5, 3, 4), (5, 3, 7), (8, 8, 8), (32, 32, 32)):
        info = _plan(f"select:{cap}", a_cap, b_cap, params=params).info()
        assert info["n_levels"] == 1 and info["n_pbs"] <= 2 * cap * BPC, (a_cap, b_cap, cap, info)
    assert _plan("select_count:16:16", params=params).info()["n_levels"] == 1


@pytest.mark.parametrize("params", (O.TOY_K1, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS), ids=lambda p: p.name)
def test_count_add_takes_no_more_levels_than_the_integer_layers_scalar_add(params):
    """The measure is read at test time: scalar_add of fhe_int_plan_create on D blocks, D the digits of the larger operand.
    Asserted on bounds that fill their D digits (n_max = 4^D - 1, D = 1 .. 4: nothing to clamp), on 5 / 4 (D = 2: the clamp sits
    inside the lookups), and on three-digit shapes whose bounds leave room in their digits: 16 / 16, 32 / 32, 48 / 63, 16 / 15,
    3 / 16, 16 / 5 and 8 / 32 with two encrypted operands, and the clear form at any bound.  There the clamp runs beside the carry
    chain: with a clear integer [a >= a_max] rides on the last lookup of every block; with two encrypted operands a three-digit
    bound that is a multiple of 16 (or fills its digits) leaves the low unit of the clamped operand zero, so its flag only gates
    the carries, and a second operand of one unit brings its clamped digits and the carries under its clamp from level 1.
    Not asserted, because it does not hold: a three-digit operand whose bound is neither, beside a second encrypted operand --
    count_add:20:20 and count_add:20:5 take 5 levels against the measure's 3 (the clamp, two levels, comes first).  With a box
    of 16 values [a >= 20] needs both units of a, so it exists after two levels at the earliest, the first carry that depends
    on it after three, and the digit above it after four."""
    import fhestr
    measure = {d: fhestr.Plan.integer_op(None, "scalar_add", d, 1, params=_params(params)).info()["n_levels"] for d in (1, 2, 3, 4)}
    for d in (1, 2, 3, 4):
        full = M ** d - 1
        assert input_digits(M, full) == d
        for op, clear in ((f"count_add:{full}:{full}", None), (f"count_add_clear:{full}", b"\x01")):
            info = _plan(op, clear=clear, params=params).info()
            assert info["n_levels"] <= measure[d], (op, info, measure[d])
    assert _plan("count_add:5:4", params=params).info()["n_levels"] <= measure[2]
    assert _plan("count_add_clear:5", clear=b"\x04", params=params).info()["n_levels"] <= measure[2]
    for a_max, b_max in ((16, 16), (32, 32), (48, 63), (16, 15), (3, 16), (16, 5), (8, 32)):
        info = _plan(f"count_add:{a_max}:{b_max}", params=params).info()
        assert info["n_levels"] <= measure[3], (a_max, b_max, info, measure[3])
    for a_max, k in ((16, 1), (16, 16), (32, 1), (20, 7), (63, 200), (100, 1)):
        d = input_digits(M, a_max)
        info = _plan(f"count_add_clear:{a_max}", clear=clear_bytes(k), params=params).info()
        assert info["n_levels"] <= measure[max(d, input_digits(M, k)) if k > a_max else d], (a_max, k, info)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

REFUSALS = [   # (op, a_cap, b_cap, clear, parameter set, what fhe_last_error names)
    ("and", 0, 0, None, O.TOY_K1, "and takes one parameter: the number of bits k"),
    ("not", 0, 0, None, O.TOY_K1, "not takes one parameter: the number of bits k"),
    ("xor:2:3", 0, 0, None, O.TOY_K1, "xor takes one parameter"),
    ("and:0", 0, 0, None, O.TOY_K1, "and: k must be at least 2"),
    ("or:1", 0, 0, None, O.TOY_K1, "or: k must be at least 2"),
    ("not:0", 0, 0, None, O.TOY_K1, "not: k must be at least 1"),
    ("and:2", 4, 0, None, O.TOY_K1, "and takes no string: a_cap and b_cap must be 0"),
    ("select", 5, 3, None, O.TOY_K1, "select takes one parameter: the output capacity C"),
    ("select:0", 5, 3, None, O.TOY_K1, "select: the output capacity must be > 0"),
    ("select_clear:0", 5, 0, b"x", O.TOY_K1, "select_clear: the output capacity must be > 0"),
    ("select:4", 0, 3, None, O.TOY_K1, "select: the string capacity must be > 0"),
    ("select:4", 5, 0, None, O.TOY_K1, "the second string needs a capacity of at least one character"),
    ("select_clear:4", 5, 3, b"x", O.TOY_K1, "b_cap must be 0"),
    ("select_count", 0, 0, None, O.TOY_K1, "select_count takes two parameters: the bounds a_max and b_max"),
    ("select_count:3", 0, 0, None, O.TOY_K1, "select_count takes two parameters"),
    ("select_count:0:3", 0, 0, None, O.TOY_K1, "select_count: a bound must be at least 1"),
    ("select_count:3:3", 2, 0, None, O.TOY_K1, "select_count takes no string"),
    ("count_add", 0, 0, None, O.TOY_K1, "count_add takes two parameters: the bounds a_max and b_max"),
    ("count_sub:5", 0, 0, None, O.TOY_K1, "count_sub takes two parameters"),
    ("count_lt:5:0", 0, 0, None, O.TOY_K1, "count_lt: a bound must be at least 1"),
    ("count_add:0:4", 0, 0, None, O.TOY_K1, "count_add: a bound must be at least 1"),
    ("count_add_clear", 0, 0, b"\x01", O.TOY_K1, "count_add_clear takes one parameter: the bound a_max"),
    ("count_eq_clear:5:4", 0, 0, b"\x01", O.TOY_K1, "count_eq_clear takes one parameter"),
    ("count_add_clear:0", 0, 0, b"\x01", O.TOY_K1, "count_add_clear: a bound must be at least 1"),
    ("count_add_clear:5", 0, 0, b"", O.TOY_K1, "the clear integer is 1 to 4 little-endian bytes, got 0"),
    ("count_ge_clear:5", 0, 0, b"\x01\x00\x00\x00\x00", O.TOY_K1, "the clear integer is 1 to 4 little-endian bytes, got 5"),
    ("count_add_clear:999999999", 0, 0, b"\xff\xff\xff\xff", O.TOY_K1, "the bound of the sum must stay below 2^32"),
    ("and_clear:2", 0, 0, b"x", O.TOY_K1, "and has no _clear form"),
    ("not_clear:1", 0, 0, b"x", O.TOY_K1, "not has no _clear form"),
    ("select_count_clear:3:3", 0, 0, b"x", O.TOY_K1, "select_count has no _clear form"),
    ("and_reference:2", 0, 0, None, O.TOY_K1, "unknown string op"),
    ("count_add:5:4", 0, 0, None, O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("count_lt_clear:5", 0, 0, b"\x01", O.TOY_K2, "needs a message * carry space of at least 16 values"),
]


@pytest.mark.parametrize("op,a_cap,b_cap,clear,params,reason", REFUSALS, ids=[f"{r[0]}-{r[1]}-{r[2]}-{r[4].name}" for r in REFUSALS])
def test_refusals_return_an_error_that_names_the_reason(op, a_cap, b_cap, clear, params, reason):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        fhestr.Plan.string_op(None, op, a_cap, b_cap, clear, params=_params(params))
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()


def test_bit_logic_and_select_build_on_a_small_box():
    """Only the count names need a box of 16 values: a gate is bit + 2 * block, which fits msg_mod * carry_mod = 4."""
    for op in ("and:2", "or:5", "xor:3", "not:2", "select_count:3:3"):
        assert _plan(op, params=O.TOY_K2).info()["n_pbs"] >= 1
    for op, b_cap, clear in (("select:4", 3, None), ("select_clear:2", 0, b"xy")):
        info = _plan(op, 5, b_cap, clear, params=O.TOY_K2).info()
        assert info["n_levels"] == 1 and info["n_outputs"] == int(op.split(":")[1]) * 8


def test_operand_kinds_are_refused_in_a_program_and_leave_it_usable():
    import fhestr
    prog = _program()
    s, t, n, c = prog.string(5), prog.string(3), prog.count(5), prog.bit()
    bit = prog.is_empty(s)
    for name, operands, clear, reason in (
            ("and:2", (bit, s), None, "and:2: operand 1 is a string: the op takes bit, bit"),
            ("and:2", (bit,), None, "and:2: takes 2 operand(s) (bit, bit), got 1"),
            ("not:1", (n,), None, "not:1: operand 0 is a count: the op takes bit"),
            ("select:4", (s, t, n), None, "select:4: operand 2 is a count: the op takes string, string, bit"),
            ("select:4", (c, s, t), None, "select:4: operand 0 is a bit: the op takes string, string, bit"),
            ("select_clear:4", (s, t, c), b"x", "select_clear:4: takes 2 operand(s) (string, bit), got 3"),
            ("select_count:5:5", (n, n), None, "select_count:5:5: takes 3 operand(s) (count, count, bit), got 2"),
            ("count_add:5:5", (n, c), None, "count_add:5:5: operand 1 is a bit: the op takes count, count"),
            ("count_add:5:5", (s, n), None, "count_add:5:5: operand 0 is a string: the op takes count, count"),
            ("count_add:3:5", (n, n), None, "count_add:3:5: the count operand has 2 digits, the op takes 1 (n_max = 3)"),
            ("count_add_clear:5", (n, n), b"\x01", "count_add_clear:5: takes 1 operand(s) (count), got 2"),
            ("count_add:5", (n, n), None, "count_add takes two parameters"),
            ("and:1", (bit,), None, "and: k must be at least 2"),
            ("count_lt_clear:5", (n,), b"", "the clear integer is 1 to 4 little-endian bytes, got 0")):
        with pytest.raises(fhestr.FheError) as err:
            prog.op(name, *operands, clear=clear)
        assert reason in str(err.value), (name, str(err.value))
    # a count of fewer digits than the name takes is extended with zero digits; the program still works
    wide = prog.op("count_add:20:5", n, n)[0]
    assert (wide.kind, wide.n_max, wide.blocks) == ("count", 25, 3)
    prog.output(prog.bit_and(bit, c), wide)
    assert prog.compile().plan.info()["n_outputs"] == 4


def test_refusals_of_the_existing_names_are_unchanged():
    """The operand rule of every other name and its texts: strings first, then at most one count."""
    import fhestr
    prog = _program()
    s, n, c = prog.string(5), prog.count(5), prog.bit()
    for name, operands, reason in (("eq", (s, c), "eq: operand 1 is a bit: an op takes its strings, then at most one count as the last operand"),
                                   ("len", (n,), "len: the first operand must be a string"),
                                   ("len", (c,), "len: operand 0 is a bit: an op takes its strings, then at most one count as the last operand"),
                                   ("to_upper", (s, n), "to_upper: takes no encrypted count"),
                                   ("take_encn:5", (s,), "take_encn:5: takes an encrypted count as its last operand"),
                                   ("eq", (n, s), "eq: operand 0 is a count: an op takes its strings, then at most one count as the last operand")):
        with pytest.raises(fhestr.FheError) as err:
            prog.op(name, *operands)
        assert reason in str(err.value), (name, str(err.value))


# ---- 1-bit blocks ---------------------------------------------------------------------------------------------------------------

P13 = dict(n=745, k=1, N=2048, pbs=(23, 1), ks=(3, 5), msg_mod=2, carry_mod=8, lwe_std=6.692125069956277e-06, glwe_std=2.9403601535432533e-16)
ONE_BIT = [("add", 20, 20, range(32), range(32)), ("sub", 40, 40, range(0, 64, 3), range(64)), ("lt", 20, 20, range(32), range(32)),
           ("add", 5, 3, range(8), range(4)), ("sub", 7, 9, range(8), range(16))]


@pytest.mark.parametrize("op,a_max,b_max,values_a,values_b", ONE_BIT, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in ONE_BIT])
def test_counts_on_one_bit_blocks(op, a_max, b_max, values_a, values_b):
    """PARAM_MESSAGE_1_CARRY_3's shape (msg_mod 2, a box of 16), offline plans on the noise-free executor (tests/clear_plan.py): a
    count of 20 travels in five digits, the radix code with a three-valued scan state in base 4.  Every pair of the values,
    those above the bounds included."""
    import fhestr
    from clear_plan import ClearBackend, run_clear
    P = fhestr.Params(P13["n"], P13["k"], P13["N"], *P13["pbs"], *P13["ks"], P13["msg_mod"], P13["carry_mod"], P13["lwe_std"], P13["glwe_std"],
                      "PARAM_MESSAGE_1_CARRY_3_KS_PBS")
    plan = fhestr.Plan.string_op(None, f"count_{op}:{a_max}:{b_max}", 0, 0, None, 1, params=P)
    noise = plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]
    backend = ClearBackend(plan, P)
    for a, b in itertools.product(values_a, values_b):
        msgs = run_clear(backend, encode_count(2, a, a_max) + encode_count(2, b, b_max))
        got = decode_bit(msgs) if op in COMPARISONS else decode_digits(msgs, 2, count_bound(op, a_max, b_max))
        assert got == count_ref(op, a, a_max, b, b_max) and backend.off_centre == 0, (op, a, b, got)
    plan.close()
