"""Combining results on the GPU -- bit logic, select, arithmetic and comparisons on counts -- PARAM_MESSAGE_2_CARRY_2 at real
dimensions with device-generated keys, against the clear-text definitions of tests/combine_ref.py: through FheStringOps,
the typed C entry point fhe_str_combine, fhe_str_plan_create + run, packed operands and results, string programs; then small
plans against the oracle-stepped plan and a toy twin with 4-bit blocks.

Shapes: strings of capacity 4 to 8; counts with the bounds 3 (one digit), 5 (two: one packed unit) and 16 (three: the radix
code)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle as O
from combine_ref import (COMPARISONS, bits_ref, clear_bytes, count_bound, count_ref, decode_bit, decode_digits, decode_string, select_count_ref,
                         select_ref)
from conftest import gpu_engine, keyset, to_fhestr_params
from count_ref import encode_count
from plan_oracle import run_with_oracle

pytestmark = pytest.mark.gpu

M, BPC = 4, 4


@pytest.fixture(scope="module")
def rig():
    """The client's own keys, the server keys generated on the device, and a packing key: once for the module."""
    import fhestr
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    assert P.msg_mod == M
    ck = fhestr.ClientKey(P, 0x5EED0C00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0C01)
    eng.load_packing_key(*ck.gen_packing_key((7, 3), seed=0x5EED0C02))
    ops = fhestr.FheStringOps(eng)
    yield P, ck, eng, ops
    ops.close()
    eng.close()
    ck.close()


def _enc(rig, s, cap):
    import fhestr
    return np.ascontiguousarray(rig[1].encrypt(fhestr.string_to_blocks(rig[0], s, cap)))


def _bit(rig, b):
    return np.ascontiguousarray(rig[1].encrypt(np.array([b], dtype=np.uint64)))


def _digits(rig, n, n_max):
    return np.ascontiguousarray(rig[1].encrypt(np.array(encode_count(M, n, n_max), dtype=np.uint64)))


def _count(rig, n, n_max):
    import fhestr
    return fhestr.EncryptedCount(_digits(rig, n, n_max), n_max)


def _dec(rig, cts):
    return [int(m) for m in rig[1].decrypt(np.asarray(cts).reshape(-1, rig[0].big_size))]


def _dec_count(rig, count):
    return decode_digits(_dec(rig, count.digits), M, count.n_max)


_ptr = lambda x: x.ctypes.data_as(C.c_void_p)


# ---- FheStringOps ---------------------------------------------------------------------------------------------------------------

def test_truth_tables_and_not(rig):
    ops = rig[3]
    for x, y in itertools.product((0, 1), repeat=2):
        bx, by = _bit(rig, x), _bit(rig, y)
        for op, call in (("and", ops.bit_and), ("or", ops.bit_or), ("xor", ops.bit_xor)):
            assert decode_bit(_dec(rig, call(bx, by))) == bits_ref(op, (x, y)), (op, x, y)
        assert _dec(rig, ops.bit_not(bx, by)) == bits_ref("not", (x, y))
    assert decode_bit(_dec(rig, ops.bit_not(_bit(rig, 0)))) == 1
    assert decode_bit(_dec(rig, ops.bit_and(_bit(rig, 1), _bit(rig, 1), _bit(rig, 0)))) == 0
    # a bit an operation returned is an operand as it is
    a = _enc(rig, b"axb", 4)
    both = ops.bit_and(ops.starts_with(a, b"a"), ops.bit_not(ops.ends_with(a, b"x")))
    assert decode_bit(_dec(rig, both)) == 1


def test_select_strings_of_unequal_capacity(rig):
    """a in 8 characters, b in 5: both branches, the default capacity (8), a cut (4) and the clear form."""
    ops = rig[3]
    for sa, sb in ((b"abcdefgh", b"xyz"), (b"ab", b"xyzuv"), (b"", b"xyz")):
        a, b = _enc(rig, sa, 8), _enc(rig, sb, 5)
        for c in (0, 1):
            cond = _bit(rig, c)
            assert decode_string(_dec(rig, ops.select(cond, a, b)), M, 8) == select_ref(c, sa, sb, 8), (sa, sb, c)
            assert decode_string(_dec(rig, ops.select(cond, a, b, out_cap=4)), M, 4) == select_ref(c, sa, sb, 4), (sa, sb, c)
            assert decode_string(_dec(rig, ops.select(cond, b, b"none!!")), M, 6) == select_ref(c, sb, b"none!!", 6), (sb, c)


def test_select_packed_operand_packed_result_and_counts(rig):
    import fhestr
    P, ck, eng, ops = rig
    a, b = _enc(rig, b"Key:Val", 8), _enc(rig, b"other", 6)
    packed_a = ops.to_lower(a, packed=True)                                                   # a PackedString operand
    assert isinstance(packed_a, fhestr.PackedString)
    for c in (0, 1):
        got = ops.select(_bit(rig, c), packed_a, b)
        assert decode_string(_dec(rig, got), M, 8) == select_ref(c, b"key:val", b"other", 8)
        packed = ops.select(_bit(rig, c), a, b, packed=True)                                  # packed=True: the result is the next operand
        assert isinstance(packed, fhestr.PackedString) and (packed.count, packed.capacity) == (8 * BPC, 8)
        assert fhestr.blocks_to_string(P, ck.decrypt_packed(packed, packed.count)) == select_ref(c, b"Key:Val", b"other", 8)
        assert decode_bit(_dec(rig, ops.eq(packed, b"Key:Val" if c else b"other"))) == 1
        for (x, x_max), (y, y_max) in (((2, 3), (11, 16)), ((16, 16), (0, 3)), ((4, 5), (5, 5))):
            got = ops.select(_bit(rig, c), _count(rig, x, x_max), _count(rig, y, y_max))
            assert got.n_max == max(x_max, y_max) and _dec_count(rig, got) == select_count_ref(c, x, y), (c, x, y)


# the carry points 3+1, 15+1, 16+16, the borrow points 4-1, 16-1, 0-1, 2-5, saturation, and operands above their bound
ARITHMETIC = [(3, (3, 3), ((3, 1), (3, 3), (0, 1), (2, 3), (0, 0))),
              (5, (5, 5), ((3, 1), (4, 1), (5, 5), (0, 1), (2, 5), (15, 1), (3, 9))),
              (16, (16, 16), ((3, 1), (15, 1), (16, 16), (4, 1), (16, 1), (0, 1), (2, 5), (16, 0), (40, 3), (7, 63))),
              (16, (16, 5), ((15, 1), (16, 5), (12, 4), (11, 5), (40, 9), (3, 15), (0, 0)))]    # three digits beside one unit


@pytest.mark.parametrize("bound,bounds,pairs", ARITHMETIC, ids=[f"bounds{a[1][0]}-{a[1][1]}" for a in ARITHMETIC])
def test_count_add_and_sub_encrypted_and_clear(rig, bound, bounds, pairs):
    ops = rig[3]
    a_max, b_max = bounds
    for a, b in pairs:
        ca, cb = _count(rig, a, a_max), _count(rig, b, b_max)
        for op, call in (("add", ops.count_add), ("sub", ops.count_sub)):
            got = call(ca, cb)
            assert got.n_max == count_bound(op, a_max, b_max) and _dec_count(rig, got) == count_ref(op, a, a_max, b, b_max), (op, a, b)
            k = min(b, b_max)                                                                 # the same second operand, clear
            got = call(ca, k)
            assert got.n_max == count_bound(op, a_max, k) and _dec_count(rig, got) == count_ref(op, a, a_max, k), (op, a, k)


@pytest.mark.parametrize("a_max,b_max", ((3, 3), (5, 16), (16, 16)))
def test_the_six_comparisons(rig, a_max, b_max):
    ops = rig[3]
    for a, b in ((1, 2), (2, 2), (3, 1), (a_max, b_max), (0, 0)):                             # a < b, a = b, a > b, the bounds
        ca, cb = _count(rig, a, a_max), _count(rig, b, b_max)
        for op in COMPARISONS:
            assert decode_bit(_dec(rig, getattr(ops, f"count_{op}")(ca, cb))) == count_ref(op, a, a_max, b, b_max), (op, a, b)
            assert decode_bit(_dec(rig, getattr(ops, f"count_{op}")(ca, b))) == count_ref(op, a, a_max, b), (op, a, b, "clear")


def test_min_and_max(rig):
    """A comparison and a select_count: operands within their bounds (select_count passes the chosen digits through)."""
    ops = rig[3]
    for a, b in ((2, 9), (5, 2), (5, 5), (4, 16)):
        ca, cb = _count(rig, a, 5), _count(rig, b, 16)
        assert _dec_count(rig, ops.count_min(ca, cb)) == min(a, b) and _dec_count(rig, ops.count_max(ca, cb)) == max(a, b)
        assert _dec_count(rig, ops.count_min(cb, 4)) == min(b, 4) and _dec_count(rig, ops.count_max(cb, 4)) == max(b, 4)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------

def test_fhe_str_combine_and_a_created_plan_decrypt_alike(rig):
    """fhe_str_combine (the output count queried with out == NULL, then the run) and fhe_str_plan_create + run on the same
    inputs: the same decryptions, and the reference's."""
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    a, b, c1 = _enc(rig, b"abcdef", 6), _enc(rig, b"xyz", 4), _bit(rig, 1)
    d5, d16, d3 = _digits(rig, 4, 5), _digits(rig, 15, 16), _digits(rig, 3, 3)
    cases = (("and:2", 0, 0, None, [c1, _bit(rig, 0)], [0]), ("xor:3", 0, 0, None, [c1, c1, c1], [1]), ("not:2", 0, 0, None, [c1, _bit(rig, 0)], [0, 1]),
             ("select:5", 6, 4, None, [a, b, c1], b"abcde"), ("select_clear:4", 6, 0, b"no", [a, _bit(rig, 0)], b"no"),
             ("select_count:5:16", 0, 0, None, [d5, d16, _bit(rig, 0)], 15), ("count_add:5:16", 0, 0, None, [d5, d16], 19),
             ("count_sub:16:5", 0, 0, None, [d16, d5], 11), ("count_lt:3:5", 0, 0, None, [d3, d5], 1),
             ("count_add_clear:16", 0, 0, clear_bytes(1), [d16], 16), ("count_ge_clear:5", 0, 0, clear_bytes(300), [d5], 0))
    for name, a_cap, b_cap, clear, operands, want in cases:
        ptrs = (C.c_void_p * len(operands))(*[x.ctypes.data for x in operands])
        counts = (C.c_uint32 * len(operands))(*[x.shape[0] for x in operands])
        buf = (C.c_uint8 * max(1, len(clear or b"")))(*(clear or b""))
        args = (eng.handle, name.encode(), ptrs, counts, len(operands), buf if clear is not None else None, len(clear or b""))
        n_out = C.c_uint32(0)
        assert L.fhe_str_combine(*args, None, C.byref(n_out)) == 0, L.fhe_last_error()
        out = np.zeros((n_out.value, P.big_size), dtype=np.uint64)
        assert L.fhe_str_combine(*args, _ptr(out), None) == 0, L.fhe_last_error()
        plan = fhestr.Plan.string_op(eng, name, a_cap, b_cap, clear)
        assert plan.info()["n_outputs"] == n_out.value
        got = _dec(rig, out)
        assert got == _dec(rig, plan.run(np.concatenate(operands))), name
        plan.close()
        if isinstance(want, bytes):
            assert decode_string(got, M, n_out.value // BPC) == want, name
        elif isinstance(want, list):
            assert got == want, name
        elif n_out.value == 1 and name.startswith(("count_lt", "count_ge")):
            assert decode_bit(got) == want, name
        else:
            assert sum(m * M ** i for i, m in enumerate(got)) == want and all(0 <= m < M for m in got), name
    # block counts are checked against the name
    n_out = C.c_uint32(0)
    for name, operands, reason in (("and:2", [c1], b"takes 2 operand(s), got 1"), ("count_add:5:16", [d5, d5], b"operand 1 has 2 blocks, the name takes a count of 3"),
                                   ("select:5", [a, b, d5], b"operand 2 has 2 blocks, the name takes a bit of 1"), ("eq", [a, b], b"not a name that combines results"),
                                   ("select:5", [d5, b, c1], b"no whole characters"), ("count_add:5", [d5, d5], b"takes two parameters")):
        ptrs = (C.c_void_p * len(operands))(*[x.ctypes.data for x in operands])
        counts = (C.c_uint32 * len(operands))(*[x.shape[0] for x in operands])
        assert L.fhe_str_combine(eng.handle, name.encode(), ptrs, counts, len(operands), None, 0, None, C.byref(n_out)) != 0, name
        assert reason in L.fhe_last_error(), L.fhe_last_error()


# ---- programs -------------------------------------------------------------------------------------------------------------------

def test_the_value_after_the_separator_end_to_end(rig):
    """The README's line: skip(kv, count_add(find(kv, ":")[1], 1)) gives b"blue" from b"colour:blue" -- stand-alone operations,
    then the same as one program."""
    import fhestr
    P, ck, eng, ops = rig
    kv = _enc(rig, b"colour:blue", 12)
    found = ops.find(kv, b":")
    index = fhestr.EncryptedCount(found[1:], 12)
    value = ops.skip(kv, ops.count_add(index, 1))
    assert decode_bit(_dec(rig, found[:1])) == 1 and decode_string(_dec(rig, value), M, 12) == b"blue"
    prog = fhestr.StringProgram(eng)
    s = prog.string(12)
    hit, at = prog.find(s, b":")
    prog.output(hit, prog.skip(s, prog.count_add(at, 1)))
    compiled = prog.compile()
    for text in (b"colour:blue", b"k:v", b":x", b"size:"):
        got = compiled(_enc(rig, text, 12))
        assert decode_bit(_dec(rig, got[0])) == 1 and decode_string(_dec(rig, got[1]), M, 12) == text.split(b":", 1)[1], text
    compiled.close()
    prog.close()


def test_program_the_shorter_string_and_a_bit_input(rig):
    import fhestr
    P, ck, eng, ops = rig
    prog = fhestr.StringProgram(eng)
    a, b, c = prog.string(6), prog.string(4), prog.bit()
    la, lb = prog.len(a), prog.len(b)
    shorter = prog.select(prog.count_lt(la, lb), a, b)
    upper = prog.select(prog.bit_and(c, prog.bit_not(prog.is_empty(a))), prog.to_upper(a), a)
    prog.output(shorter, prog.count_min(la, lb), upper)
    compiled = prog.compile()
    for sa, sb, bit in ((b"abc", b"xy", 1), (b"ab", b"xyz", 0), (b"", b"x", 1), (b"abcdef", b"", 1), (b"ab", b"xy", 0), (b"a", b"xyzw", 1)):
        got = compiled(_enc(rig, sa, 6), _enc(rig, sb, 4), _bit(rig, bit))
        assert decode_string(_dec(rig, got[0]), M, 6) == (sa if len(sa) < len(sb) else sb), (sa, sb)
        assert _dec_count(rig, got[1]) == min(len(sa), len(sb)), (sa, sb)
        assert decode_string(_dec(rig, got[2]), M, 6) == (sa.upper() if bit else sa), (sa, bit)
    compiled.close()
    prog.close()


# ---- against the oracle-stepped plan --------------------------------------------------------------------------------------------

ORACLE_CASES = [   # (plan name, a_cap, b_cap, clear, the clear inputs in plan order): small plans, the oracle steps every lookup on the CPU
    ("and:2", 0, 0, None, [[1], [1]]), ("not:1", 0, 0, None, [[0]]), ("select:1", 1, 1, None, [[1, 2, 0, 0], [2, 3, 0, 0], [0]]),
    ("count_add:5:4", 0, 0, None, [encode_count(M, 3, 5), encode_count(M, 4, 4)]), ("count_sub:3:3", 0, 0, None, [[1], [3]]),
    ("count_lt_clear:5", 0, 0, b"\x04", [encode_count(M, 9, 5)]),
]


@pytest.mark.parametrize("name,a_cap,b_cap,clear,clear_inputs", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_gpu_plan_decrypts_like_the_oracle_stepped_plan(p22, name, a_cap, b_cap, clear, clear_inputs):
    import fhestr
    eng = gpu_engine(p22)
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    inputs = np.concatenate([p22.ck.encrypt_many(np.array(x, dtype=np.uint64)) for x in clear_inputs])
    gpu = fhestr.Plan.string_op(eng, name, a_cap, b_cap, clear).run(inputs)
    cpu = run_with_oracle(fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, params=P), inputs, p22.sk)
    got = p22.ck.decrypt_many(np.asarray(gpu).reshape(-1, P.big_size)).tolist()
    assert got == p22.ck.decrypt_many(cpu).tolist()
    want = {"and:2": [1], "not:1": [1], "select:1": [2, 3, 0, 0], "count_add:5:4": encode_count(M, 7, 9), "count_sub:3:3": [0], "count_lt_clear:5": [0]}
    assert got == want[name]


@pytest.mark.parametrize("name,clear", (("xor:2", None), ("select:3", None), ("count_add:9:30", None), ("count_sub_clear:40", b"\x07"),
                                        ("count_add:256:16", None), ("count_sub:300:20", None), ("count_sub_clear:256", b"\x07"), ("count_add_clear:300", b"\x07")))
def test_toy_twin_with_4_bit_blocks(name, clear):
    """msg_mod = carry_mod = 16: two blocks per character, a count up to 15 is one digit.  The GPU run decrypts like the
    oracle-stepped plan, and to the reference."""
    import fhestr
    ks = keyset(O.TOY_N32768)
    eng = gpu_engine(ks)
    P = eng.params
    a_cap, b_cap = (3, 2) if name.startswith("select") else (0, 0)
    plans = fhestr.Plan.string_op(eng, name, a_cap, b_cap, clear), fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, params=to_fhestr_params(O.TOY_N32768))
    enc = lambda values: ks.ck.encrypt_many(np.array(values, dtype=np.uint64))
    cases = {"xor:2": [([[1], [1]], [0]), ([[0], [1]], [1])],
             "select:3": [([fhestr.string_to_blocks(P, b"abc", 3), fhestr.string_to_blocks(P, b"x", 2), [c]], list(fhestr.string_to_blocks(P, w, 3)))
                          for c, w in ((1, b"abc"), (0, b"x"))],
             "count_add:9:30": [([encode_count(16, a, 9), encode_count(16, b, 30)], encode_count(16, min(a, 9) + min(b, 30), 39))
                                for a, b in ((9, 30), (15, 1), (3, 200))],
             "count_sub_clear:40": [([encode_count(16, a, 40)], encode_count(16, max(min(a, 40) - 7, 0), 40)) for a in (40, 6, 16, 255)],
             # three digits of 4 bits: the clamp beside the carry chain, the comparator on single blocks, the two-step fix-up
             "count_add:256:16": [([encode_count(16, a, 256), encode_count(16, b, 16)], encode_count(16, min(a, 256) + min(b, 16), 272))
                                  for a, b in ((255, 1), (256, 16), (4095, 255), (15, 15), (240, 16))],
             "count_sub:300:20": [([encode_count(16, a, 300), encode_count(16, b, 20)], encode_count(16, max(min(a, 300) - min(b, 20), 0), 300))
                                  for a, b in ((256, 1), (300, 20), (4095, 255), (5, 19), (272, 17))],
             "count_sub_clear:256": [([encode_count(16, a, 256)], encode_count(16, max(min(a, 256) - 7, 0), 256)) for a in (256, 6, 263, 4095)],
             "count_add_clear:300": [([encode_count(16, a, 300)], encode_count(16, min(a, 300) + 7, 307)) for a in (300, 249, 255, 4095)]}[name]
    for clear_inputs, want in cases:
        inputs = np.concatenate([enc(x) for x in clear_inputs])
        got = ks.ck.decrypt_many(np.asarray(plans[0].run(inputs)).reshape(-1, ks.params.big_size)).tolist()
        assert got == ks.ck.decrypt_many(run_with_oracle(plans[1], inputs, ks.sk)).tolist(), (name, clear_inputs)
        assert got == [int(w) for w in want], (name, clear_inputs, got)
    for plan in plans:
        plan.close()
