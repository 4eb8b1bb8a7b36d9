"""take, skip, split_at, char_at and insert at a clear or an ENCRYPTED position, without a GPU: the C++ planner builds
offline plans on TOY_K1 (msg_mod = 4), the CPU oracle executes their exported levels, results are compared with the
clear-text definitions of tests/slice_ref.py.

An encrypted position travels in D base-4 digits, D the smallest with 4^D > n_max; a value above the bound must act as the
bound.  At a_cap = n_max = 8 that is two digits -- one packed unit -- and n runs over 0 .. 15."""
import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from count_ref import encode_count, input_digits
from plan_oracle import run_with_oracle
from slice_ref import (char_at_ref, decode_slice, insert_ref, skip_ref, slice_ref, split_at_ref, substring_ref, take_ref)
from test_count_cpu import _run_two_ranks

A_CAP = 8
M = O.TOY_K1.msg_mod
BPC = 4
OPS = ("take", "skip", "split_at", "char_at", "insert")
STRINGS = [b"", b"a", b"abcd", b"abcdefgh"]             # empty, one character, len = 4, full capacity with no padding
T_ENC, T_CAP = b"XY", 3                                # the encrypted string of insert: hidden length 2 in capacity 3


def _params(p=O.TOY_K1):
    return to_fhestr_params(p)


_PLANS = {}


def _plan(op, a_cap, b_cap=0, clear=None, world=1, params=None):
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


def _slice(ks, op, s, n, a_cap=A_CAP, n_max=None, cap=None, t=None, t_cap=None, world=1, run=run_with_oracle):
    """The decoded result of `op` on s at position n: encrypted with the bound n_max, or clear (n_max=None).  t: the string
    insert takes, encrypted in t_cap characters or clear (t_cap=None)."""
    enc_t = op == "insert" and t_cap is not None
    clear = t if op == "insert" and not enc_t else None
    name = (op + ("_encn" if n_max is not None else "") + ("_clear" if clear is not None else "") +
            f":{n if n_max is None else n_max}" + (f":{cap}" if cap is not None else ""))
    plan = _plan(name, a_cap, t_cap if enc_t else 0, clear, world)
    out_cap = cap if cap is not None else a_cap + ((t_cap if enc_t else len(t)) if op == "insert" else 0)
    n_strings = {"split_at": 2, "char_at": 0}.get(op, 1)
    assert plan.info()["n_outputs"] == (1 + BPC if op == "char_at" else n_strings * out_cap * BPC), name
    operands = [_enc(ks, s, a_cap)] + ([_enc(ks, t, t_cap)] if enc_t else []) + ([_enc_count(ks, n, n_max)] if n_max is not None else [])
    assert plan.info()["n_inputs"] == sum(len(x) for x in operands), name
    return decode_slice(op, ks.ck.decrypt_many(run(plan, np.concatenate(operands), ks.sk)), M, out_cap)


def _want(op, s, n, n_max=None, cap=None, t=b"", t_cap=None, a_cap=A_CAP):
    if cap is None:
        cap = a_cap + ((t_cap if t_cap is not None else len(t)) if op == "insert" else 0)
    return slice_ref(op, s, n, n_max, cap, t)


# ---- encrypted positions ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
def test_every_position_offline_plan_vs_reference(toy_k1, op):
    """a_cap = n_max = 8: two digits, one packed unit; every n in 0 .. 15, so 9 .. 15 lie above the bound and act as 8."""
    assert input_digits(M, 8) == 2
    kw = dict(t=T_ENC, t_cap=T_CAP) if op == "insert" else {}
    for s in STRINGS:
        for n in range(M ** 2):
            got = _slice(toy_k1, op, s, n, n_max=8, **kw)
            assert got == _want(op, s, n, 8, **kw), (op, s, n, got)
    assert take_ref(b"abcd", 9, 3) == b"abc" and skip_ref(b"abcd", 2, 8) == b"cd" and char_at_ref(b"abcd", 4, 8) == (0, b"")
    assert insert_ref(b"abcd", 15, b"XY", 8) == b"abcdXY" and split_at_ref(b"abcd", 1, 8) == (b"a", b"bcd")


@pytest.mark.parametrize("op", OPS)
def test_odd_capacity_the_top_stage_runs_off_the_end(toy_k1, op):
    """a_cap = 5: the shifter's stage by 4 keeps one character, every other one is gated."""
    kw = dict(t=T_ENC, t_cap=T_CAP) if op == "insert" else {}
    for s in (b"", b"ab", b"abcde"):
        for n in range(8):
            got = _slice(toy_k1, op, s, n, a_cap=5, n_max=5, **kw)
            assert got == _want(op, s, n, 5, a_cap=5, **kw), (op, s, n, got)


@pytest.mark.parametrize("op", OPS)
def test_three_digit_position_takes_the_sign_tree(toy_k1, op):
    """a_cap = n_max = 20: three digits, two packed units, the multi-unit comparison."""
    assert input_digits(M, 20) == 3
    kw = dict(t=T_ENC, t_cap=T_CAP) if op == "insert" else {}
    for s in (b"abcdefghijklmnopqrst", b"abcdefg"):
        for n in (0, 1, 19, 20, 21, 63):
            got = _slice(toy_k1, op, s, n, a_cap=20, n_max=20, **kw)
            assert got == _want(op, s, n, 20, a_cap=20, **kw), (op, s, n, got)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n_max", [5, 13], ids=["below_a_cap", "above_a_cap"])
def test_bound_below_and_above_the_capacity(toy_k1, op, n_max):
    kw = dict(t=T_ENC, t_cap=T_CAP) if op == "insert" else {}
    for s in (b"abcdefgh", b"abcde", b""):
        for n in sorted({0, 2, n_max - 1, n_max, n_max + 1, M ** input_digits(M, n_max) - 1}):
            got = _slice(toy_k1, op, s, n, n_max=n_max, **kw)
            assert got == _want(op, s, n, n_max, **kw), (op, s, n, n_max, got)


@pytest.mark.parametrize("op", ("take", "skip", "split_at", "insert"))
@pytest.mark.parametrize("cap", [3, 13], ids=["below_default", "above_default"])
def test_output_capacities(toy_k1, op, cap):
    """Cut or zero padded to C; an insert whose result overflows C is cut."""
    kw = dict(t=T_ENC, t_cap=T_CAP) if op == "insert" else {}
    for s in (b"abcdefgh", b"abc"):
        for n in (0, 2, 5, 8, 12):
            got = _slice(toy_k1, op, s, n, n_max=8, cap=cap, **kw)
            assert got == _want(op, s, n, 8, cap=cap, **kw), (op, s, n, cap, got)
        for n in (0, 2, 8, 9):
            assert _slice(toy_k1, op, s, n, cap=cap, **kw) == _want(op, s, n, cap=cap, **kw), (op, s, n, cap)
    assert insert_ref(b"abcdefgh", 2, b"XY", 8, 3) == b"abX"


def test_insert_encrypted_clear_and_empty(toy_k1):
    """t encrypted with a hidden length, filling its capacity, all padding; clear; clear and empty; and a full string, whose
    result overflows the default capacity only where t fills its own."""
    for s in (b"abcd", b"abcdefgh", b""):
        for n in (0, 1, 4, 8, 11):
            for t, t_cap in ((b"XY", 3), (b"XYZ", 3), (b"", 2), (b"XY", None), (b"", None)):
                got = _slice(toy_k1, "insert", s, n, n_max=8, t=t, t_cap=t_cap)
                assert got == _want("insert", s, n, 8, t=t, t_cap=t_cap), (s, n, t, t_cap, got)
    for t, t_cap in ((b"XYZ", 3), (b"XYZ", None)):           # 11 characters cut at 8
        assert _slice(toy_k1, "insert", b"abcdefgh", 3, n_max=8, cap=8, t=t, t_cap=t_cap) == b"abcXYZde"


# ---- clear positions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
def test_clear_positions(toy_k1, op):
    """Mostly rewiring: n = 0, inside, n = a_cap and n > a_cap; the plans still build and run."""
    for t, t_cap in (((b"XY", 3), (b"XY", None), (b"", None)) if op == "insert" else ((b"", None),)):
        kw = dict(t=t, t_cap=t_cap) if op == "insert" else {}
        for s in STRINGS:
            for n in (0, 3, A_CAP, A_CAP + 3):
                got = _slice(toy_k1, op, s, n, **kw)
                assert got == _want(op, s, n, **kw), (op, s, n, t, t_cap, got)


def test_split_at_parts_equal_take_and_skip(toy_k1):
    for s in STRINGS:
        for n, n_max in ((3, 8), (11, 8), (0, 8), (5, None), (0, None), (9, None)):
            parts = _slice(toy_k1, "split_at", s, n, n_max=n_max)
            assert parts == (_slice(toy_k1, "take", s, n, n_max=n_max), _slice(toy_k1, "skip", s, n, n_max=n_max)), (s, n, n_max)


# ---- cost ---------------------------------------------------------------------------------------------------------------------

def test_char_at_is_not_a_shifter():
    for a_cap in (8, 20, 32):
        for params in (O.TOY_K1, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS):
            char_at = _plan(f"char_at_encn:{a_cap}", a_cap, params=params).info()["n_pbs"]
            skip = _plan(f"skip_encn:{a_cap}", a_cap, params=params).info()["n_pbs"]
            assert char_at < skip, (a_cap, params.name, char_at, skip)


def test_skip_is_a_shifter_by_the_bits_of_the_position():
    """a_cap = n_max = 20: no more than ceil(log2 20) = 5 stages of one lookup per string block, the decoding of the
    position (what the same name costs at a_cap = 1 bounds it) and one cleaning lookup per block.  An indicator that
    shifts along with the string costs a lookup per character and stage more."""
    for params in (O.TOY_K1, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS):
        n_pbs = _plan("skip_encn:20", 20, params=params).info()["n_pbs"]
        decoding = _plan("skip_encn:20", 1, params=params).info()["n_pbs"]
        assert n_pbs <= 5 * 20 * BPC + decoding + 20 * BPC, (params.name, n_pbs, decoding)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

REFUSALS = [   # (op, b_cap, clear, parameter set, what fhe_last_error names)
    ("take_encn:0", 0, None, O.TOY_K1, "n_max must be at least 1"),
    ("skip_encn:0:4", 0, None, O.TOY_K1, "n_max must be at least 1"),
    ("split_at_encn:0", 0, None, O.TOY_K1, "n_max must be at least 1"),
    ("char_at_encn:0", 0, None, O.TOY_K1, "n_max must be at least 1"),
    ("insert_encn:0", 2, None, O.TOY_K1, "n_max must be at least 1"),
    ("insert_encn_clear:0", 0, b"x", O.TOY_K1, "n_max must be at least 1"),
    ("take:3:0", 0, None, O.TOY_K1, "output capacity must be > 0"),
    ("skip_encn:3:0", 0, None, O.TOY_K1, "output capacity must be > 0"),
    ("split_at:3:0", 0, None, O.TOY_K1, "output capacity must be > 0"),
    ("insert_clear:3:0", 0, b"x", O.TOY_K1, "output capacity must be > 0"),
    ("take", 0, None, O.TOY_K1, "takes one or two parameters: the position n"),
    ("skip_encn", 0, None, O.TOY_K1, "takes one or two parameters: the position's bound n_max"),
    ("split_at", 0, None, O.TOY_K1, "takes one or two parameters"),
    ("char_at", 0, None, O.TOY_K1, "takes one parameter: the position n"),
    ("insert", 2, None, O.TOY_K1, "takes one or two parameters"),
    ("insert_encn_clear", 0, b"x", O.TOY_K1, "takes one or two parameters"),
    ("take:1:2:3", 0, None, O.TOY_K1, "takes one or two parameters"),
    ("char_at:3:4", 0, None, O.TOY_K1, "there is no output capacity"),
    ("char_at_encn:3:4", 0, None, O.TOY_K1, "there is no output capacity"),
    ("take_clear:3", 0, b"x", O.TOY_K1, "_clear is a form of insert only"),
    ("insert:3", 0, None, O.TOY_K1, "pattern capacity must be > 0"),
    ("take_encn:3", 0, None, O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("skip_encn:3", 0, None, O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("split_at_encn:3", 0, None, O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("char_at_encn:3", 0, None, O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("insert_encn_clear:3", 0, b"x", O.TOY_K2, "needs a message * carry space of at least 16 values"),
    ("take:3", 0, None, O.TOY_N8192, "msg_mod = 2^b with b | 8"),
    ("skip_encn:3", 0, None, O.TOY_N8192, "msg_mod = 2^b with b | 8"),
]


@pytest.mark.parametrize("op,b_cap,clear,params,reason", REFUSALS, ids=[f"{r[0]}-{r[3].name}" for r in REFUSALS])
def test_refusals_return_an_error_that_names_the_reason(op, b_cap, clear, params, reason):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        fhestr.Plan.string_op(None, op, A_CAP, b_cap, clear, params=_params(params))
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()


def test_clear_positions_build_on_a_small_box_and_every_capacity_builds():
    """The clear-position forms need no 16-value box (insert is a concat, which TOY_K2's noise budget of 9 variances does not
    admit); the bound may exceed the capacity; capacities that are no power of two and 4-bit blocks (two per character)
    build within the noise budget."""
    for op in ("take:3", "skip:3", "split_at:3", "char_at:3"):
        _plan(op, A_CAP, params=O.TOY_K2)
    for params in (O.TOY_K1, O.TOY_N32768, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS):
        for a_cap in (1, 2, 3, 5, 7, 12, 33):
            for n_max in (1, a_cap, 2 * a_cap + 1):
                for op in OPS:
                    _plan(f"{op}_encn:{n_max}", a_cap, 2 if op == "insert" else 0, params=params)
    assert _plan("skip_encn:300", 4).info()["n_inputs"] == 4 * BPC + input_digits(M, 300)


# ---- two ranks ----------------------------------------------------------------------------------------------------------------

def test_world_2_build_decrypts_to_the_same_outputs(toy_k1):
    for n in (0, 3, 7, 12):
        for s in (b"abcdefgh", b"abcde"):
            assert _slice(toy_k1, "skip", s, n, n_max=8, world=2, run=_run_two_ranks) == skip_ref(s, n, 8), (s, n)
            got = _slice(toy_k1, "insert", s, n, n_max=8, t=T_ENC, t_cap=T_CAP, world=2, run=_run_two_ranks)
            assert got == insert_ref(s, n, T_ENC, 8, A_CAP + T_CAP), (s, n, got)


# ---- programs -----------------------------------------------------------------------------------------------------------------

def _program():
    import fhestr
    return fhestr.StringProgram(None, params=_params())


def _run_program(ks, compiled, inputs):
    import fhestr
    msgs = ks.ck.decrypt_many(run_with_oracle(compiled.plan, np.concatenate(inputs), ks.sk)).reshape(-1, 1)
    return tuple(int(np.asarray(x).reshape(-1)[0]) if np.asarray(x).size == 1 else fhestr.blocks_to_string(_params(), x)
                 for x in compiled.results_of(msgs))


def test_program_skip_at_the_index_of_find(toy_k1):
    """s[find(s, ":") + 0:] with no glue: find's index (n_max = a_cap) is the count operand of skip_encn:<a_cap>."""
    prog = _program()
    s = prog.string(A_CAP)
    found, index = prog.find(s, b":")
    assert (index.kind, index.n_max) == ("count", A_CAP)
    rest = prog.skip(s, index)
    assert (rest.kind, rest.cap) == ("string", A_CAP)
    prog.output(found, rest)
    compiled = prog.compile()
    for text in (b"key:val", b":abc", b"abcdefg:", b"no colon", b""):
        at = text.find(b":")
        want = (int(at >= 0), text[at:] if at >= 0 else text)        # (not found: the index is 0)
        assert _run_program(toy_k1, compiled, [_enc(toy_k1, text, A_CAP)]) == want, text


def test_program_take_the_length_of_another_string(toy_k1):
    """The first len(t) characters of s: len's count (n_max = the capacity of t) feeds take_encn."""
    prog = _program()
    s, t = prog.string(A_CAP), prog.string(5)
    head = prog.take(s, prog.len(t))
    valid, ch = prog.char_at(s, prog.len(t))
    assert (head.cap, valid.kind, ch.cap) == (A_CAP, "bit", 1)
    prog.output(head, valid, ch)
    compiled = prog.compile()
    for text, other in ((b"abcdefgh", b"xyz"), (b"ab", b"xyzuv"), (b"abcdefgh", b""), (b"", b"xy")):
        want = (text[:len(other)],) + char_at_ref(text, len(other))
        assert _run_program(toy_k1, compiled, [_enc(toy_k1, text, A_CAP), _enc(toy_k1, other, 5)]) == want, (text, other)


def test_program_substring_is_one_plan(toy_k1):
    import fhestr
    prog = _program()
    s, start, length = prog.string(A_CAP), prog.count(8), prog.count(3)
    prog.output(prog.substring(s, start, length), prog.substring(s, 2, 3), prog.insert(s, start, b"--", out_cap=6))
    assert prog.n_ops == 5
    compiled = prog.compile()
    for text in (b"abcdefgh", b"abc", b""):
        for a, n in ((0, 0), (1, 2), (3, 3), (7, 3), (8, 1), (13, 2)):
            inputs = [_enc(toy_k1, text, A_CAP), _enc_count(toy_k1, a, 8), _enc_count(toy_k1, n, 3)]
            want = (substring_ref(text, min(a, 8), n), text[2:5], insert_ref(text, a, b"--", 8, 6))
            assert _run_program(toy_k1, compiled, inputs) == want, (text, a, n)
    with pytest.raises(fhestr.FheError, match="digits"):        # the count's digits must fit the name's bound
        p2 = _program()
        p2.op("take_encn:3", p2.string(A_CAP), p2.count(8))
