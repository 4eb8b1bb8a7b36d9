"""repeat, replacen, splitn and rsplitn with an ENCRYPTED count on the GPU, PARAM_MESSAGE_2_CARRY_2 at real dimensions,
against the clear-text definitions of tests/count_ref.py: through the C entry points, through FheStringOps (fresh
digits, and the digits `len` returns), packed results as operands, many rows with one shared count, and against the
oracle-stepped plan.

msg_mod = 4.  n_max = 3 travels in D = 1 digit and 3 is also the largest value the digit holds, so n runs over 0 .. 3;
the clamp runs with n_max = 2 and n = 3."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import gpu_engine, to_fhestr_params
from count_ref import encode_count, repeat_ref, replacen_ref, splitn_ref
from plan_oracle import run_with_oracle
from split_ref import decode_split

pytestmark = pytest.mark.gpu

A_CAP, N_MAX, M = 8, 3, 4
# (string, pattern): the comma strings and the self-overlapping separators, 1- and 2-character patterns
CASES = [(b"a,b,c,d", b","), (b",a,b", b","), (b"a,,b", b","), (b"", b","), (b"abc", b","), (b"aaaa", b"aa"), (b"aaa", b"aa"),
         (b"abababa", b"ab")]
SPLITS = ("splitn", "rsplitn")


@pytest.fixture(scope="module")
def rig():
    """The client's own keys, the server keys generated on the device, and a packing key (packed results go back in as
    operands): once for the module."""
    import fhestr
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    assert P.msg_mod == M
    ck = fhestr.ClientKey(P, 0x5EED0E00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0E01)
    eng.load_packing_key(*ck.gen_packing_key((7, 3), seed=0x5EED0E02))
    ops = fhestr.FheStringOps(eng)
    yield P, ck, eng, ops
    ops.close()
    eng.close()
    ck.close()


def _enc(rig, s, cap):
    import fhestr
    P, ck = rig[0], rig[1]
    return np.ascontiguousarray(ck.encrypt(fhestr.string_to_blocks(P, s, cap)))


def _digits(rig, n, n_max):
    import fhestr
    digits = fhestr.encode_count(rig[0], n, n_max)
    assert digits.tolist() == encode_count(M, n, n_max)
    return np.ascontiguousarray(rig[1].encrypt(digits))


def _count(rig, n, n_max=N_MAX):
    import fhestr
    return fhestr.EncryptedCount(_digits(rig, n, n_max), n_max)


def _dec(rig, cts):
    return rig[1].decrypt(np.asarray(cts).reshape(-1, rig[0].big_size))


def _string(rig, cts):
    import fhestr
    return fhestr.blocks_to_string(rig[0], _dec(rig, cts))


def _split_decoded(rig, res, max_parts, part_cap=A_CAP):
    flat = np.concatenate([np.asarray(res.count).reshape(-1, rig[0].big_size)] + [np.asarray(p) for p in res.parts])
    return decode_split("splitn", _dec(rig, flat), M, max_parts, part_cap)


_ptr = lambda x: x.ctypes.data_as(C.c_void_p)
_bytes = lambda b: (C.c_uint8 * max(1, len(b)))(*b)


# ---- the C entry points -----------------------------------------------------------------------------------------------------

def test_fhe_str_repeat(rig):
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    for s in (b"ab", b"a,b,c,d", b"abcdefgh", b""):
        a = _enc(rig, s, A_CAP)
        for n in range(4):
            out = np.zeros((N_MAX * A_CAP * 4, P.big_size), dtype=np.uint64)
            assert L.fhe_str_repeat(eng.handle, _ptr(a), A_CAP, _ptr(_digits(rig, n, N_MAX)), N_MAX, _ptr(out)) == 0, L.fhe_last_error()
            assert _string(rig, out) == repeat_ref(s, n, N_MAX), (s, n)
    assert L.fhe_str_repeat(eng.handle, _ptr(a), A_CAP, _ptr(_digits(rig, 1, 3)), 0, _ptr(out)) != 0
    assert b"1..255" in L.fhe_last_error()


@pytest.mark.parametrize("op", SPLITS)
def test_fhe_str_splitn_encn(rig, op):
    """The output count queried with out == NULL, then the run; part_cap 0 = a_cap; clear and encrypted patterns."""
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    for s, sep in CASES:
        a = _enc(rig, s, A_CAP)
        pat = _enc(rig, sep, len(sep))
        for encrypted in (False, True):
            head = (eng.handle, op.encode(), _ptr(a), A_CAP, _ptr(pat) if encrypted else None, len(sep) if encrypted else 0,
                    None if encrypted else _bytes(sep), 0 if encrypted else len(sep))
            n_out = C.c_uint32(0)
            assert L.fhe_str_splitn_encn(*head, None, N_MAX, 0, None, C.byref(n_out)) == 0, L.fhe_last_error()
            assert n_out.value == 2 + N_MAX * A_CAP * 4          # the layout of splitn:3 -- P + 1 = 4 needs two base-4 digits
            for n in range(4):
                out = np.zeros((n_out.value, P.big_size), dtype=np.uint64)
                assert L.fhe_str_splitn_encn(*head, _ptr(_digits(rig, n, N_MAX)), N_MAX, 0, _ptr(out), None) == 0, L.fhe_last_error()
                got = decode_split("splitn", _dec(rig, out), M, N_MAX, A_CAP)
                assert got == splitn_ref(op, s, sep, n, N_MAX), (op, s, sep, encrypted, n, got)
    n_out = C.c_uint32(0)
    assert L.fhe_str_splitn_encn(eng.handle, b"split", _ptr(a), A_CAP, None, 0, _bytes(b","), 1, None, 2, 0, None, C.byref(n_out)) != 0
    assert b"splitn" in L.fhe_last_error()
    assert L.fhe_str_splitn_encn(eng.handle, op.encode(), _ptr(a), A_CAP, None, 0, _bytes(b""), 0, None, 2, 0, None, C.byref(n_out)) != 0
    assert b"must not be empty" in L.fhe_last_error()


def test_fhe_str_replacen_encn(rig):
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    out_cap = 12
    for s, frm in CASES:
        to = b"xyz"
        a, f, t = _enc(rig, s, A_CAP), _enc(rig, frm, 2), _enc(rig, to, 3)      # `from` zero padded to capacity 2
        for n in range(4):
            d = _digits(rig, n, N_MAX)
            want = replacen_ref(s, frm, to, n, N_MAX, out_cap)                  # (b"axyzbxyzcxyzd" is cut at 12 characters)
            out = np.zeros((out_cap * 4, P.big_size), dtype=np.uint64)
            assert L.fhe_str_replacen_encn_clear(eng.handle, _ptr(a), A_CAP, _bytes(frm), len(frm), _bytes(to), len(to), _ptr(d), N_MAX,
                                                 out_cap, _ptr(out)) == 0, L.fhe_last_error()
            assert _string(rig, out) == want, (s, frm, n, "clear")
            out = np.zeros((out_cap * 4, P.big_size), dtype=np.uint64)
            assert L.fhe_str_replacen_encn(eng.handle, _ptr(a), A_CAP, _ptr(f), 2, _ptr(t), 3, _ptr(d), N_MAX, out_cap, _ptr(out)) == 0, L.fhe_last_error()
            assert _string(rig, out) == want, (s, frm, n, "encrypted")
    assert L.fhe_str_replacen_encn_clear(eng.handle, _ptr(a), A_CAP, _bytes(b""), 0, _bytes(b"x"), 1, _ptr(d), N_MAX, out_cap, _ptr(out)) != 0
    assert b"must not be empty" in L.fhe_last_error()


# ---- FheStringOps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ("repeat", "replacen") + SPLITS)
def test_ops_with_fresh_digits(rig, op):
    """Clear patterns and encrypted ones zero padded to capacity 2."""
    P, ck, eng, ops = rig
    for s, sep in CASES:
        a = _enc(rig, s, A_CAP)
        pat = _enc(rig, sep, 2)
        for n in range(4):
            count = _count(rig, n)
            if op == "repeat":
                out = ops.repeat(a, count)
                assert out.shape == (N_MAX * A_CAP * 4, P.big_size) and _string(rig, out) == repeat_ref(s, n, N_MAX), (s, n)
            elif op == "replacen":
                want = replacen_ref(s, sep, b"-", n, N_MAX)
                assert _string(rig, ops.replacen(a, sep, b"-", count)) == want, (s, sep, n)
                assert _string(rig, ops.replacen(a, pat, _enc(rig, b"-", 1), count)) == want, (s, sep, n)
            else:
                for p in (sep, pat):
                    res = getattr(ops, op)(a, p, count)
                    assert len(res.parts) == N_MAX
                    assert _split_decoded(rig, res, N_MAX) == splitn_ref(op, s, sep, n, N_MAX), (op, s, sep, n, type(p))


def test_the_bound_clamps_the_count(rig):
    """n_max = 2 and n = 3 (one digit holds it): the operations act as for n = 2."""
    a = _enc(rig, b"a,b,c,d", A_CAP)
    count = _count(rig, 3, n_max=2)
    ops = rig[3]
    assert _string(rig, ops.repeat(a, count)) == b"a,b,c,d" * 2 == repeat_ref(b"a,b,c,d", 3, 2)
    assert _split_decoded(rig, ops.splitn(a, b",", count), 2) == (2, [b"a", b"b,c,d"]) == splitn_ref("splitn", b"a,b,c,d", b",", 3, 2)
    assert _split_decoded(rig, ops.rsplitn(a, b",", count), 2) == (2, [b"d", b"a,b,c"]) == splitn_ref("rsplitn", b"a,b,c,d", b",", 3, 2)
    assert _string(rig, ops.replacen(a, b",", b";", count)) == b"a;b;c,d" == replacen_ref(b"a,b,c,d", b",", b";", 3, 2)


def test_the_digits_of_len_are_a_count(rig):
    """ops.len(b) of a capacity-8 string returns two digits: they go in as they are, with a two-digit bound (n_max = 4)."""
    import fhestr
    P, ck, eng, ops = rig
    a = _enc(rig, b"a,b,c,d", A_CAP)
    short = _enc(rig, b"xy", 2)
    for b in (b"", b"ab", b"abc", b"abcdefg"):
        count = fhestr.EncryptedCount(ops.len(_enc(rig, b, A_CAP)), 4)
        n = len(b)
        assert _string(rig, ops.repeat(short, count)) == repeat_ref(b"xy", n, 4), b
        assert _split_decoded(rig, ops.splitn(a, b",", count), 4) == splitn_ref("splitn", b"a,b,c,d", b",", n, 4), b
        assert _split_decoded(rig, ops.rsplitn(a, _enc(rig, b",", 1), count), 4) == splitn_ref("rsplitn", b"a,b,c,d", b",", n, 4), b
        assert _string(rig, ops.replacen(a, b",", b"--", count, out_cap=12)) == replacen_ref(b"a,b,c,d", b",", b"--", n, 4), b
    assert fhestr.EncryptedCount(ops.len(a), params=P).n_max == 15
    with pytest.raises(fhestr.FheError, match="digits"):
        ops.repeat(short, fhestr.EncryptedCount(ops.len(a), 3))             # two digits, but n_max = 3 travels in one


def test_packed_results_are_operands(rig):
    import fhestr
    P, ck, eng, ops = rig
    s = b"ab,c,,d"
    a = _enc(rig, s, A_CAP)
    n_blocks = A_CAP * 4
    packed_a = ops.to_lower(a, packed=True)                                  # a PackedString operand
    for n in range(4):
        count = _count(rig, n)
        want_count, want_parts = splitn_ref("splitn", s, b",", n, N_MAX)
        res = ops.splitn(packed_a, b",", count, packed=True)
        assert isinstance(res.count, fhestr.PackedString) and fhestr.decode_count(P, ck.decrypt_packed(res.count, 2)) == want_count
        for part, want in zip(res.parts, want_parts):
            assert isinstance(part, fhestr.PackedString) and (part.count, part.capacity) == (n_blocks, A_CAP)
            assert fhestr.blocks_to_string(P, ck.decrypt_packed(part, n_blocks)) == want
        # a returned part straight into the next operation
        assert ck.decrypt(ops.eq(res.parts[0], b"ab").reshape(1, -1))[0] == int(want_parts[0] == b"ab")
        assert ck.decrypt(ops.eq(res.parts[1], b"c,,d").reshape(1, -1))[0] == int(want_parts[1] == b"c,,d")
        res = ops.rsplitn(a, _enc(rig, b",", 1), count, packed=True)
        assert [fhestr.blocks_to_string(P, ck.decrypt_packed(p, n_blocks)) for p in res.parts] == splitn_ref("rsplitn", s, b",", n, N_MAX)[1]
        rep = ops.repeat(packed_a, count, packed=True)
        assert (rep.count, rep.capacity) == (N_MAX * n_blocks, N_MAX * A_CAP)
        assert fhestr.blocks_to_string(P, ck.decrypt_packed(rep, rep.count)) == repeat_ref(s, n, N_MAX)
        out = ops.replacen(res.parts[0], b",", b"+", count, packed=True)
        assert fhestr.blocks_to_string(P, ck.decrypt_packed(out, n_blocks)) == replacen_ref(splitn_ref("rsplitn", s, b",", n, N_MAX)[1][0], b",", b"+", n, N_MAX)
    # the count itself may come packed: the digits of len
    count = fhestr.EncryptedCount(ops.len(_enc(rig, b"xy", A_CAP), packed=True), 4)
    assert _string(rig, ops.repeat(_enc(rig, b"ab", 2), count)) == b"abab"


def test_op_many_three_rows_share_one_count(rig):
    P, ck, eng, ops = rig
    texts = [b"a,b,c,d", b",,", b"abc"]
    rows = np.stack([_enc(rig, t, A_CAP) for t in texts])
    for n in (0, 2, 3):
        count = _count(rig, n)
        many = ops.op_many(f"repeat:{N_MAX}", rows, count=count)
        assert many.shape == (3, N_MAX * A_CAP * 4, P.big_size)
        assert [_string(rig, m) for m in many] == [repeat_ref(t, n, N_MAX) for t in texts]
        many = ops.op_many(f"splitn_encn:{N_MAX}", rows, b",", count=count)              # clear bytes: splitn_encn_clear is meant
        assert [decode_split("splitn", _dec(rig, m), M, N_MAX, A_CAP) for m in many] == [splitn_ref("splitn", t, b",", n, N_MAX) for t in texts]
        many = ops.op_many(f"rsplitn_encn:{N_MAX}", rows, _enc(rig, b",", 2), count=count)    # the pattern, then the digits, shared
        assert [decode_split("splitn", _dec(rig, m), M, N_MAX, A_CAP) for m in many] == [splitn_ref("rsplitn", t, b",", n, N_MAX) for t in texts]
        many = ops.op_many(f"replacen_encn:{N_MAX}:1:{A_CAP}", rows, b",;", count=count)
        assert [_string(rig, m) for m in many] == [replacen_ref(t, b",", b";", n, N_MAX) for t in texts]
    import fhestr
    per_row = N_MAX * A_CAP * 4
    packed = ops.op_many(f"repeat:{N_MAX}", rows, count=_count(rig, 2), packed=True)     # the device route shares the digits too
    msgs = ck.decrypt_packed(packed, 3 * per_row)
    assert [fhestr.blocks_to_string(P, msgs[r * per_row:(r + 1) * per_row]) for r in range(3)] == [repeat_ref(t, 2, N_MAX) for t in texts]


# ---- against the oracle-stepped plan ----------------------------------------------------------------------------------------

ORACLE_CASES = [   # (plan name, a_cap, clear, string, n): small shapes, the oracle steps every lookup on the CPU
    ("repeat:2", 2, None, b"ab", 2),
    ("splitn_encn_clear:2", 3, b",", b"a,b", 2),
    ("rsplitn_encn_clear:2", 3, b",", b"a,b", 1),
    ("replacen_encn_clear:2:1:4", 4, b",;", b"a,b,", 1),
]


@pytest.mark.parametrize("name,a_cap,clear,s,n", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_gpu_plan_decrypts_like_the_oracle_stepped_plan(p22, name, a_cap, clear, s, n):
    import fhestr
    eng = gpu_engine(p22)
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    inputs = np.concatenate([p22.ck.encrypt_many(fhestr.string_to_blocks(P, s, a_cap)),
                             p22.ck.encrypt_many(np.array(encode_count(M, n, 2), dtype=np.uint64))])
    gpu = fhestr.Plan.string_op(eng, name, a_cap, 0, clear).run(inputs)
    cpu = run_with_oracle(fhestr.Plan.string_op(None, name, a_cap, 0, clear, params=P), inputs, p22.sk)
    got = p22.ck.decrypt_many(np.asarray(gpu).reshape(-1, P.big_size)).tolist()
    assert got == p22.ck.decrypt_many(cpu).tolist()
    if name.startswith("repeat"):
        assert fhestr.blocks_to_string(P, got) == repeat_ref(s, n, 2)
    elif "splitn" in name:
        assert decode_split("splitn", got, M, 2, a_cap) == splitn_ref(name.split("_")[0], s, clear, n, 2)
    else:
        assert fhestr.blocks_to_string(P, got) == replacen_ref(s, clear[:1], clear[1:], n, 2)
