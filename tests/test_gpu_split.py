"""The split family and replacen on the GPU against the clear-text definitions of tests/split_ref.py:
through FheStringOps and through fhe_str_split directly, clear and encrypted patterns, PARAM_MESSAGE_2_CARRY_2
at 32 characters, parts that come back packed and go into the next operation, and many rows per pass."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import gpu_engine, to_fhestr_params
from plan_oracle import run_with_oracle
from split_ref import ONCE, decode_split, split_ref

pytestmark = pytest.mark.gpu

A_CAP = 8


def _enc(ks, s: bytes, cap: int):
    import fhestr
    return ks.ck.encrypt_many(fhestr.string_to_blocks(gpu_engine(ks).params, s, cap))


def _dec(ks, cts):
    return ks.ck.decrypt_many(np.asarray(cts).reshape(-1, ks.params.big_size))


def _ops(ks):
    import fhestr
    return fhestr.FheStringOps(gpu_engine(ks))


def _decoded(ks, op, res, max_parts, part_cap):
    """(count, parts) of a SplitResult with expanded members."""
    head = np.asarray(res.count).reshape(-1, ks.params.big_size)
    flat = np.concatenate([head] + [np.asarray(p) for p in res.parts])
    return decode_split(op, _dec(ks, flat), ks.params.msg_mod, max_parts, part_cap)


def _call(ops, op, a, pat, max_parts, part_cap=None):
    if op == "split_ascii_whitespace":
        return ops.split_ascii_whitespace(a, max_parts, part_cap)
    if op in ONCE:
        return getattr(ops, op)(a, pat, part_cap)
    return getattr(ops, op)(a, pat, max_parts, part_cap)


TOY_CASES = [   # (op, s, sep, max_parts, part_cap)
    ("split", b"a,b,c,d", b",", 3, None),               # more parts than max_parts: count == 4
    ("split", b",a,,b", b",", 3, None),
    ("rsplit", b"aaa", b"aa", 2, None),                 # cut from the right: ["", "a"] with the "a" in front
    ("split", b"aaa", b"aa", 2, None),
    ("split_terminator", b"a,b,", b",", 3, None),
    ("rsplit_terminator", b"abababa", b"aba", 2, None),
    ("split_inclusive", b"a,,b", b",", 3, None),
    ("splitn", b"a,b,c,d", b",", 2, None),
    ("rsplitn", b"a,b,c,d", b",", 2, None),
    ("split_once", b"k=v=w", b"=", 2, None),
    ("rsplit_once", b"k=v=w", b"=", 2, None),
    ("split_once", b"abc", b"=", 2, None),              # not found: (s, "")
    ("split", b"abc,d,ef", b",", 2, 2),                 # parts cut at two characters
    ("split", b"", b",", 2, None),
    ("split_ascii_whitespace", b" a\t\nb ", None, 2, None),
    ("split_ascii_whitespace", b"a b c d", None, 3, 1),
]


@pytest.mark.parametrize("op,s,sep,max_parts,part_cap", TOY_CASES)
def test_split_family_clear_and_encrypted_patterns(toy_k1, op, s, sep, max_parts, part_cap):
    ops = _ops(toy_k1)
    want = split_ref(op, s, sep, max_parts, part_cap=part_cap)
    a = _enc(toy_k1, s, A_CAP)
    patterns = [None] if sep is None else [sep, _enc(toy_k1, sep, len(sep)), _enc(toy_k1, sep, 4)]       # clear, encrypted, padded
    for pat in patterns:
        res = _call(ops, op, a, pat, max_parts, part_cap)
        assert len(res.parts) == max_parts and all(p.shape == ((part_cap or A_CAP) * 4, toy_k1.params.big_size) for p in res.parts)
        assert _decoded(toy_k1, op, res, max_parts, part_cap or A_CAP) == want, (op, s, type(pat))


def test_fhe_str_split_directly(toy_k1):
    """The C entry point as a C caller uses it: the output count queried with out == NULL, then the run; part_cap 0 = a_cap."""
    import fhestr
    eng = gpu_engine(toy_k1)
    L = fhestr.lib()
    big = toy_k1.params.big_size
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    for op, s, sep, enc_cap, max_parts, part_cap in (("rsplit", b"a,b,,c", b",", None, 3, 0), ("split_inclusive", b"xabyab", b"ab", 4, 2, 0),
                                                     ("rsplit_once", b"a=b=c", b"=", None, 7, 3), ("split_ascii_whitespace", b"ab  cd e", None, None, 2, 4)):
        a = np.ascontiguousarray(_enc(toy_k1, s, A_CAP))
        pat = np.ascontiguousarray(_enc(toy_k1, sep, enc_cap)) if enc_cap else None
        clear = (C.c_uint8 * len(sep))(*sep) if sep is not None and not enc_cap else None
        args = (eng.handle, op.encode(), ptr(a), A_CAP, ptr(pat) if enc_cap else None, enc_cap or 0, clear, len(sep) if clear is not None else 0,
                max_parts, part_cap)
        n_out = C.c_uint32(0)
        assert L.fhe_str_split(*args, None, C.byref(n_out)) == 0, L.fhe_last_error()
        P = 2 if op in ONCE else max_parts
        head = 1 if op in ONCE else 1 + (max_parts + 1 >= 4)
        assert n_out.value == head + P * (part_cap or A_CAP) * 4
        out = np.zeros((n_out.value, big), dtype=np.uint64)
        assert L.fhe_str_split(*args, ptr(out), None) == 0, L.fhe_last_error()
        got = decode_split(op, _dec(toy_k1, out), 4, P, part_cap or A_CAP)
        assert got == split_ref(op, s, sep, P, part_cap=part_cap or None), (op, got)
    # refusals come back as errors with the reason
    a = np.ascontiguousarray(_enc(toy_k1, b"abc", A_CAP))
    n_out = C.c_uint32(0)
    empty = (C.c_uint8 * 1)()
    assert L.fhe_str_split(eng.handle, b"split", ptr(a), A_CAP, None, 0, empty, 0, 2, 0, None, C.byref(n_out)) != 0
    assert b"must not be empty" in L.fhe_last_error()
    assert L.fhe_str_split(eng.handle, b"splitn", ptr(a), A_CAP, None, 0, empty, 1, 0, 0, None, C.byref(n_out)) != 0
    assert b"n must be at least 1" in L.fhe_last_error()
    assert L.fhe_str_split(eng.handle, b"split_ascii_whitespace", ptr(a), A_CAP, None, 0, empty, 1, 2, 0, None, C.byref(n_out)) != 0
    assert b"takes no pattern" in L.fhe_last_error()
    assert L.fhe_str_split(eng.handle, b"explode", ptr(a), A_CAP, None, 0, empty, 1, 2, 0, None, C.byref(n_out)) != 0
    assert b"unknown operation" in L.fhe_last_error()


def test_gpu_plan_decrypts_like_the_oracle_stepped_plan(toy_k1):
    import fhestr
    eng = gpu_engine(toy_k1)
    P = to_fhestr_params(O.TOY_K1)
    inputs = np.concatenate([_enc(toy_k1, b"abxabyab", A_CAP), _enc(toy_k1, b"ab", 4)])
    gpu = fhestr.Plan.string_op(eng, "rsplit_terminator:3", A_CAP, 4).run(inputs)
    cpu = run_with_oracle(fhestr.Plan.string_op(None, "rsplit_terminator:3", A_CAP, 4, params=P), inputs, toy_k1.sk)
    assert _dec(toy_k1, gpu).tolist() == _dec(toy_k1, cpu).tolist()
    assert decode_split("rsplit_terminator", _dec(toy_k1, gpu), 4, 3, A_CAP) == split_ref("rsplit_terminator", b"abxabyab", b"ab", 3)


@pytest.mark.parametrize("s,frm,to,n", [(b"abcabc", b"bc", b"XY", 1), (b"aaaa", b"a", b"bc", 2), (b"abababab", b"aba", b"x", 5), (b"hello", b"l", b"", 0)])
def test_replacen(toy_k1, s, frm, to, n):
    import fhestr
    ops = _ops(toy_k1)
    P = gpu_engine(toy_k1).params
    a = _enc(toy_k1, s, A_CAP)
    want = s.replace(frm, to, n)
    assert fhestr.blocks_to_string(P, _dec(toy_k1, ops.replacen(a, frm, to, n, out_cap=10))) == want
    out = ops.replacen(a, _enc(toy_k1, frm, 4), _enc(toy_k1, to, 2), n, out_cap=10)
    assert out.shape == (10 * 4, toy_k1.params.big_size)
    assert fhestr.blocks_to_string(P, _dec(toy_k1, out)) == want


def test_op_many_split_equals_single_calls(toy_k1):
    ops = _ops(toy_k1)
    texts = [b"a,b,c,d", b",,", b"abc"]
    rows = np.stack([_enc(toy_k1, t, A_CAP) for t in texts])
    many = ops.op_many("split_clear:3", rows, b",")
    assert many.shape == (3, 2 + 3 * A_CAP * 4, toy_k1.params.big_size)
    for r, t in enumerate(texts):
        single = ops.split(rows[r], b",", 3)
        flat = np.concatenate([single.count] + single.parts)
        assert _dec(toy_k1, many[r]).tolist() == _dec(toy_k1, flat).tolist()
        assert decode_split("split", _dec(toy_k1, many[r]), 4, 3, A_CAP) == split_ref("split", t, b",", 3)
    assert np.array_equal(_dec(toy_k1, ops.op_many("split:3", rows, b",")), _dec(toy_k1, many))      # the same plan, named without _clear


# ---- PARAM_MESSAGE_2_CARRY_2, 32 characters ---------------------------------------------------------------------------
LINE = b"the quick  brown fox,jumps"
P22_CASES = [("split", b" ", 4), ("rsplitn", b" ", 2), ("split_once", b",", 2), ("split_ascii_whitespace", None, 4)]


@pytest.mark.parametrize("op,sep,max_parts", P22_CASES)
def test_p22_split_32_chars(p22, op, sep, max_parts):
    ops = _ops(p22)
    res = _call(ops, op, _enc(p22, LINE, 32), sep, max_parts)
    assert _decoded(p22, op, res, max_parts, 32) == split_ref(op, LINE, sep, max_parts)


def test_p22_replacen_32_chars(p22):
    import fhestr
    ops = _ops(p22)
    out = ops.replacen(_enc(p22, LINE, 32), b"o", b"0", 1)
    assert fhestr.blocks_to_string(gpu_engine(p22).params, _dec(p22, out)) == LINE.replace(b"o", b"0", 1)


@pytest.fixture(scope="module")
def packing_rig():
    """PARAM_MESSAGE_2_CARRY_2 with the client's own keys, the server keys generated on the device, and a packing key of
    three levels (packed results go back in as operands)."""
    import fhestr
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    ck = fhestr.ClientKey(P, 0x5EED0D00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0D01)
    eng.load_packing_key(*ck.gen_packing_key((7, 3), seed=0x5EED0D02))
    ops = fhestr.FheStringOps(eng)
    yield P, ck, eng, ops
    ops.close()
    eng.close()
    ck.close()


def test_p22_packed_parts_are_operands(packing_rig):
    import fhestr
    P, ck, eng, ops = packing_rig
    n_blocks = 32 * ops.bpc
    a = ck.encrypt(fhestr.string_to_blocks(P, LINE, 32))
    want_count, want_parts = split_ref("split", LINE, b" ", 4)
    res = ops.split(a, b" ", 4, packed=True)
    assert isinstance(res.count, fhestr.PackedString) and res.count.count == 2
    assert fhestr.decode_count(P, ck.decrypt_packed(res.count, 2)) == want_count == 5
    assert len(res.parts) == 4
    for part, want in zip(res.parts, want_parts):
        assert isinstance(part, fhestr.PackedString) and (part.count, part.capacity) == (n_blocks, 32) and part.shape == (1, P.k + 1, P.N)
        assert fhestr.blocks_to_string(P, ck.decrypt_packed(part, n_blocks)) == want
    # a packed part straight into the next operation
    assert ck.decrypt(ops.eq(res.parts[0], b"the").reshape(1, -1))[0] == 1
    assert ck.decrypt(ops.eq(res.parts[1], b"the").reshape(1, -1))[0] == 0
    # a packed string in, expanded parts out; found is one block
    tail = ops.rsplitn(a, b" ", 2, packed=True).parts[0]
    once = ops.split_once(tail, b",", part_cap=8)
    assert ck.decrypt(once.found.reshape(1, -1))[0] == 1
    assert [fhestr.blocks_to_string(P, ck.decrypt(p)) for p in once.parts] == [b"fox", b"jumps"]
