"""take, skip, split_at, char_at and insert at clear and ENCRYPTED positions on the GPU, PARAM_MESSAGE_2_CARRY_2 at real
dimensions with device-generated keys, against the clear-text definitions of tests/slice_ref.py: through FheStringOps,
the typed C entry point, fhe_str_op by name, op_many with a shared position, packed results as operands, a PackedString
operand and a string program; then a toy twin with 4-bit blocks and small plans against the oracle-stepped plan."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import gpu_engine, keyset, to_fhestr_params
from count_ref import encode_count
from plan_oracle import run_with_oracle
from slice_ref import char_at_ref, decode_slice, insert_ref, skip_ref, slice_ref, split_at_ref, substring_ref, take_ref

pytestmark = pytest.mark.gpu

M, BPC = 4, 4
OPS = ("take", "skip", "split_at", "char_at", "insert")
# (capacity = n_max, the positions, the strings): two digits / one packed unit, and three digits / the sign tree
SHAPES = [(8, (0, 3, 8, 11), (b"abcdefgh", b"abcde", b"")), (20, (0, 7, 20, 40), (b"abcdefghijklmnopqrst", b"abcdefghijk"))]
T_ENC, T_CAP = b"XY", 3


@pytest.fixture(scope="module")
def rig():
    """The client's own keys, the server keys generated on the device, and a packing key: once for the module."""
    import fhestr
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    assert P.msg_mod == M
    ck = fhestr.ClientKey(P, 0x5EED0F00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0F01)
    eng.load_packing_key(*ck.gen_packing_key((7, 3), seed=0x5EED0F02))
    ops = fhestr.FheStringOps(eng)
    yield P, ck, eng, ops
    ops.close()
    eng.close()
    ck.close()


def _enc(rig, s, cap):
    import fhestr
    return np.ascontiguousarray(rig[1].encrypt(fhestr.string_to_blocks(rig[0], s, cap)))


def _digits(rig, n, n_max):
    import fhestr
    digits = fhestr.encode_count(rig[0], n, n_max)
    assert digits.tolist() == encode_count(M, n, n_max)
    return np.ascontiguousarray(rig[1].encrypt(digits))


def _count(rig, n, n_max):
    import fhestr
    return fhestr.EncryptedCount(_digits(rig, n, n_max), n_max)


def _dec(rig, cts):
    return rig[1].decrypt(np.asarray(cts).reshape(-1, rig[0].big_size))


def _flat(out):
    return np.concatenate([np.asarray(x).reshape(-1, np.asarray(x).shape[-1]) for x in out]) if isinstance(out, tuple) else out


_ptr = lambda x: x.ctypes.data_as(C.c_void_p)
_bytes = lambda b: (C.c_uint8 * max(1, len(b)))(*b)


def _call(ops, op, a, n, t=None):
    return _flat(getattr(ops, op)(a, n, t) if op == "insert" else getattr(ops, op)(a, n))


# ---- FheStringOps -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap,positions,strings", SHAPES, ids=["a_cap8", "a_cap20"])
@pytest.mark.parametrize("op", OPS)
def test_ops_at_encrypted_positions(rig, op, cap, positions, strings):
    t = _enc(rig, T_ENC, T_CAP) if op == "insert" else None
    out_cap = cap + (T_CAP if op == "insert" else 0)
    for s in strings:
        a = _enc(rig, s, cap)
        for n in positions:
            got = decode_slice(op, _dec(rig, _call(rig[3], op, a, _count(rig, n, cap), t)), M, out_cap)
            assert got == slice_ref(op, s, n, cap, out_cap, T_ENC), (op, s, n, got)


@pytest.mark.parametrize("op", OPS)
def test_ops_at_clear_positions_and_a_clear_insert(rig, op):
    """The clear-position plans are mostly rewiring; they run like any other plan.  insert: a clear t, and an empty one."""
    cap = 8
    for s in (b"abcdefgh", b"abc"):
        a = _enc(rig, s, cap)
        for n in (0, 3, 8, 11):
            for t in ((b"XY", b"") if op == "insert" else (None,)):
                out_cap = cap + len(t or b"")
                got = decode_slice(op, _dec(rig, _call(rig[3], op, a, n, t)), M, out_cap)
                assert got == slice_ref(op, s, n, None, out_cap, t or b""), (op, s, n, t, got)
    if op == "insert":
        got = decode_slice(op, _dec(rig, rig[3].insert(a, _count(rig, 2, 8), b"XY")), M, 10)
        assert got == insert_ref(b"abc", 2, b"XY", 8) == b"abXYc"


def test_output_capacity_substring_and_truncate(rig):
    P, ck, eng, ops = rig
    a = _enc(rig, b"key:value", 12)
    assert decode_slice("skip", _dec(rig, ops.skip(a, _count(rig, 4, 12), out_cap=5)), M, 5) == b"value"
    assert decode_slice("take", _dec(rig, ops.truncate(a, _count(rig, 3, 12), out_cap=14)), M, 14) == b"key"
    assert decode_slice("insert", _dec(rig, ops.insert(a, _count(rig, 3, 12), _enc(rig, b"--", 2), out_cap=6)), M, 6) == b"key--:"
    got = ops.substring(a, _count(rig, 4, 12), _count(rig, 3, 12))
    assert decode_slice("take", _dec(rig, got), M, 12) == substring_ref(b"key:value", 4, 3) == b"val"
    assert decode_slice("take", _dec(rig, ops.substring(a, 1, 2)), M, 12) == b"ey"


def test_slice_at_the_index_find_returns(rig):
    """s[find(s, ":") + 0:] without a round trip: the index digits of find are the position as they are."""
    import fhestr
    P, ck, eng, ops = rig
    for s in (b"key:value", b":abc", b"abcdefghijk:"):
        a = _enc(rig, s, 12)
        found = ops.find(a, b":")
        at = fhestr.EncryptedCount(found[1:], 12)
        assert int(_dec(rig, found[:1])[0]) == 1
        assert decode_slice("skip", _dec(rig, ops.skip(a, at)), M, 12) == s[s.find(b":"):]
        assert decode_slice("char_at", _dec(rig, _flat(ops.char_at(a, at))), M, 1) == (1, b":")
        assert decode_slice("take", _dec(rig, ops.take(a, fhestr.EncryptedCount(ops.len(_enc(rig, b"xyz", 12)), 12))), M, 12) == s[:3]


# ---- the C entry points -------------------------------------------------------------------------------------------------------

def test_fhe_str_slice(rig):
    """The output count queried with out == NULL, then the run: clear and encrypted positions, encrypted and clear t."""
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    cap, s = 8, b"abcde"
    a, t = _enc(rig, s, cap), _enc(rig, T_ENC, T_CAP)
    for op in OPS:
        for n, n_max in ((3, None), (11, None), (3, 8), (11, 8)):
            for t_form in (("enc", "clear") if op == "insert" else (None,)):
                d = _digits(rig, n, n_max) if n_max else None
                head = (eng.handle, op.encode(), _ptr(a), cap, _ptr(t) if t_form == "enc" else None, T_CAP if t_form == "enc" else 0,
                        _bytes(b"-+") if t_form == "clear" else None, 2 if t_form == "clear" else 0, _ptr(d) if n_max else None, n_max or n, 0)
                n_out = C.c_uint32(0)
                assert L.fhe_str_slice(*head, None, C.byref(n_out)) == 0, L.fhe_last_error()
                out_cap = cap + {"enc": T_CAP, "clear": 2, None: 0}[t_form]
                assert n_out.value == {"split_at": 2 * cap * BPC, "char_at": 1 + BPC}.get(op, out_cap * BPC)
                out = np.zeros((n_out.value, P.big_size), dtype=np.uint64)
                assert L.fhe_str_slice(*head, _ptr(out), None) == 0, L.fhe_last_error()
                want = slice_ref(op, s, n, n_max, out_cap, T_ENC if t_form == "enc" else b"-+")
                assert decode_slice(op, _dec(rig, out), M, out_cap) == want, (op, n, n_max, t_form)
    out = np.zeros((5 * BPC, P.big_size), dtype=np.uint64)
    assert L.fhe_str_slice(eng.handle, b"skip", _ptr(a), cap, None, 0, None, 0, _ptr(_digits(rig, 2, 8)), 8, 5, _ptr(out), None) == 0, L.fhe_last_error()
    assert decode_slice("skip", _dec(rig, out), M, 5) == b"cde"
    n_out = C.c_uint32(0)
    for args, reason in (((b"split", None, 0, None, 0, None, 3, 0), b"op must be"), ((b"take", _ptr(t), T_CAP, None, 0, None, 3, 0), b"only insert"),
                         ((b"take_encn", None, 0, None, 0, None, 3, 0), b"op must be"), ((b"char_at", None, 0, None, 0, None, 3, 4), b"no output capacity"),
                         ((b"skip", None, 0, None, 0, _ptr(_digits(rig, 1, 3)), 0, 0), b"n_max must be at least 1")):
        assert L.fhe_str_slice(eng.handle, args[0], _ptr(a), cap, *args[1:], None, C.byref(n_out)) != 0
        assert reason in L.fhe_last_error(), L.fhe_last_error()


def test_fhe_str_op_by_name(rig):
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    cap, s = 8, b"abcdefgh"
    a, t, d = _enc(rig, s, cap), _enc(rig, T_ENC, T_CAP), _digits(rig, 5, 8)
    for name, operands, digits, clear, op, out_cap, want in (
            ("skip_encn:8", [a], d, None, "skip", 8, b"fgh"), ("take:3:4", [a], None, None, "take", 4, b"abc"),
            ("insert_encn:8:9", [a, t], d, None, "insert", 9, b"abcdeXYfg"), ("insert_clear:8", [a], None, b"!", "insert", 9, b"abcdefgh!"),
            ("char_at_encn:8", [a], d, None, "char_at", 1, (1, b"f")), ("split_at_encn:8:6", [a], d, None, "split_at", 6, (b"abcde", b"fgh"))):
        ptrs = (C.c_void_p * len(operands))(*[x.ctypes.data for x in operands])
        caps = (C.c_uint32 * len(operands))(*[x.shape[0] // BPC for x in operands])
        args = (eng.handle, name.encode(), ptrs, caps, len(operands), _ptr(digits) if digits is not None else None,
                _bytes(clear) if clear is not None else None, len(clear or b""))
        n_out = C.c_uint32(0)
        assert L.fhe_str_op(*args, None, C.byref(n_out)) == 0, L.fhe_last_error()
        out = np.zeros((n_out.value, P.big_size), dtype=np.uint64)
        assert L.fhe_str_op(*args, _ptr(out), None) == 0, L.fhe_last_error()
        assert decode_slice(op, _dec(rig, out), M, out_cap) == want, name


# ---- many rows, packed results and operands -----------------------------------------------------------------------------------

def test_op_many_four_rows_share_one_position(rig):
    import fhestr
    P, ck, eng, ops = rig
    texts = [b"abcdefgh", b"ab:cd", b"", b"abc"]
    rows = np.stack([_enc(rig, s, 8) for s in texts])
    for n in (0, 3, 11):
        many = ops.op_many("skip_encn:8", rows, count=_count(rig, n, 8))
        assert many.shape == (4, 8 * BPC, P.big_size)
        assert [decode_slice("skip", _dec(rig, m), M, 8) for m in many] == [skip_ref(s, n, 8) for s in texts], n
    many = ops.op_many("insert_encn:8", rows, b"+", count=_count(rig, 2, 8))                 # clear bytes: insert_encn_clear is meant
    assert [decode_slice("insert", _dec(rig, m), M, 9) for m in many] == [insert_ref(s, 2, b"+", 8) for s in texts]
    many = ops.op_many("take:2", rows)
    assert [decode_slice("take", _dec(rig, m), M, 8) for m in many] == [s[:2] for s in texts]
    packed = ops.op_many("skip_encn:8", rows, count=_count(rig, 1, 8), packed=True)          # the device route shares the digits too
    msgs = ck.decrypt_packed(packed, 4 * 8 * BPC)
    assert [fhestr.blocks_to_string(P, msgs[r * 32:(r + 1) * 32]) for r in range(4)] == [s[1:] for s in texts]


def test_packed_results_are_operands(rig):
    import fhestr
    P, ck, eng, ops = rig
    s, cap = b"key:val", 8
    a = _enc(rig, s, cap)
    packed_a = ops.to_lower(a, packed=True)                                                  # a PackedString operand
    for n in (0, 3, 9):
        head, tail = ops.split_at(packed_a, _count(rig, n, 8), packed=True)                  # each part packed on its own
        for part, want in zip((head, tail), split_at_ref(s, n, 8)):
            assert isinstance(part, fhestr.PackedString) and (part.count, part.capacity) == (cap * BPC, cap)
            assert fhestr.blocks_to_string(P, ck.decrypt_packed(part, cap * BPC)) == want
            assert ck.decrypt(ops.eq(part, want + b"x").reshape(1, -1))[0] == 0               # a part straight into the next operation
            assert ck.decrypt(ops.eq(part, _enc(rig, want, cap)).reshape(1, -1))[0] == 1
    rest = ops.skip(packed_a, 4, packed=True)
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(rest, rest.count)) == b"val"
    got = ops.char_at(packed_a, _count(rig, 3, 8), packed=True)
    assert decode_slice("char_at", ck.decrypt_packed(got, 1 + BPC), M, 1) == (1, b":")
    narrow = ops.take(a, _count(rig, 3, 8), packed=fhestr.Narrow())                          # a NarrowString result, then operand
    assert isinstance(narrow, fhestr.NarrowString)
    assert decode_slice("insert", _dec(rig, ops.insert(narrow, 1, b"-")), M, 9) == b"k-ey"
    # the position itself may come packed: the digits of len
    at = fhestr.EncryptedCount(ops.len(_enc(rig, b"xyzw", 8), packed=True), 8)
    assert decode_slice("skip", _dec(rig, ops.skip(a, at)), M, 8) == b"val"


def test_program_skips_to_the_index_of_find(rig):
    import fhestr
    P, ck, eng, ops = rig
    prog = fhestr.StringProgram(eng)
    s = prog.string(12)
    found, index = prog.find(s, b":")
    valid, ch = prog.char_at(s, index)
    prog.output(found, prog.skip(s, index), valid, ch, prog.substring(s, index, 3))
    compiled = prog.compile()
    for text in (b"key:value", b":abc", b"abcdefghijk:", b"no colon"):
        got = compiled(_enc(rig, text, 12))
        at = max(text.find(b":"), 0)                                                          # (not found: the index is 0)
        assert int(_dec(rig, got[0])[0]) == int(b":" in text)
        assert decode_slice("skip", _dec(rig, got[1]), M, 12) == text[at:]
        assert decode_slice("char_at", _dec(rig, np.concatenate([got[2].reshape(1, -1), got[3]])), M, 1) == char_at_ref(text, at)
        assert decode_slice("take", _dec(rig, got[4]), M, 12) == text[at:at + 3]
    compiled.close()
    prog.close()


# ---- against the oracle-stepped plan ------------------------------------------------------------------------------------------

ORACLE_CASES = [   # (plan name, a_cap, b_cap, clear, string, n, n_max): small shapes, the oracle steps every lookup on the CPU
    ("take_encn:2", 2, 0, None, b"ab", 1, 2), ("skip_encn:3", 3, 0, None, b"abc", 2, 3), ("char_at_encn:3", 3, 0, None, b"ab", 1, 3),
    ("split_at_encn:2", 2, 0, None, b"ab", 3, 2), ("insert_encn_clear:2", 2, 0, b"-", b"ab", 1, 2), ("skip:1", 2, 0, None, b"ab", 1, None),
]


@pytest.mark.parametrize("name,a_cap,b_cap,clear,s,n,n_max", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_gpu_plan_decrypts_like_the_oracle_stepped_plan(p22, name, a_cap, b_cap, clear, s, n, n_max):
    import fhestr
    eng = gpu_engine(p22)
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    inputs = p22.ck.encrypt_many(fhestr.string_to_blocks(P, s, a_cap))
    if n_max:
        inputs = np.concatenate([inputs, p22.ck.encrypt_many(np.array(encode_count(M, n, n_max), dtype=np.uint64))])
    gpu = fhestr.Plan.string_op(eng, name, a_cap, b_cap, clear).run(inputs)
    cpu = run_with_oracle(fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, params=P), inputs, p22.sk)
    got = p22.ck.decrypt_many(np.asarray(gpu).reshape(-1, P.big_size)).tolist()
    assert got == p22.ck.decrypt_many(cpu).tolist()
    op = name.split(":")[0].replace("_clear", "").replace("_encn", "")
    out_cap = a_cap + len(clear or b"")
    assert decode_slice(op, got, M, out_cap) == slice_ref(op, s, n, n_max, out_cap, clear or b"")


@pytest.mark.parametrize("op", ("take", "skip", "char_at"))
def test_toy_twin_with_4_bit_blocks(op):
    """msg_mod = carry_mod = 16: two blocks per character, select_block falls back to two gates, char_is_zero is one lookup.
    The GPU run decrypts like the oracle-stepped plan, and to the reference."""
    import fhestr
    ks = keyset(O.TOY_N32768)
    eng = gpu_engine(ks)
    P, cap = eng.params, 5
    name = f"{op}_encn:{cap}"
    plans = fhestr.Plan.string_op(eng, name, cap), fhestr.Plan.string_op(None, name, cap, params=to_fhestr_params(O.TOY_N32768))
    for s, n in ((b"abcde", 2), (b"abc", 4), (b"abcde", 9)):
        inputs = np.concatenate([ks.ck.encrypt_many(fhestr.string_to_blocks(P, s, cap)),
                                 ks.ck.encrypt_many(np.array(encode_count(16, n, cap), dtype=np.uint64))])
        got = ks.ck.decrypt_many(np.asarray(plans[0].run(inputs)).reshape(-1, ks.params.big_size)).tolist()
        assert got == ks.ck.decrypt_many(run_with_oracle(plans[1], inputs, ks.sk)).tolist(), (op, s, n)
        assert decode_slice(op, got, 16, cap) == slice_ref(op, s, n, cap, cap), (op, s, n)
    for plan in plans:
        plan.close()
