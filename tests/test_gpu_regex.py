"""matches on the GPU against Python's `re` (the translation of tests/regex_ref.py): PARAM_MESSAGE_2_CARRY_2 with
device-generated keys at 12 characters, through FheStringOps, through fhe_str_matches_clear directly, with a packed
operand and a packed result, and many ragged rows per pass."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from regex_ref import has_match

pytestmark = pytest.mark.gpu

A_CAP = 12


@pytest.fixture(scope="module")
def rig():
    """The client's own keys, the server keys generated on the device, and a packing key of three levels."""
    import fhestr
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    ck = fhestr.ClientKey(P, 0x5EED0E00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0E01)
    eng.load_packing_key(*ck.gen_packing_key((7, 3), seed=0x5EED0E02))
    ops = fhestr.FheStringOps(eng)
    yield P, ck, eng, ops
    ops.close()
    eng.close()
    ck.close()


def _enc(rig, s: bytes, cap=A_CAP):
    import fhestr
    P, ck, _, _ = rig
    return ck.encrypt(fhestr.string_to_blocks(P, s, cap))


# every AST node and both anchors: (pattern, strings)
CASES = [
    (b"/a.c/", [b"xxabcxx", b"ac", b""]),                                                # any character
    (b"/^[0-9]*$/", [b"4453", b"445a", b"", b"012345678901"]),                           # range, *, both anchors, nullable
    (b"/[a-z]+@[a-z]+/", [b"me@host.org", b"@host", b"me@", b"a@b"]),                    # + twice, a plain symbol
    (b"/ab|cd|ef/i", [b"xxCd", b"aceb", b"xxxxxxxxxxEF"]),                               # alternation of three, /i
    (b"/^(ab|c)+d?$/", [b"abcabd", b"abcabdd", b"cccccccccccc", b"d"]),                  # group, ?, both anchors
    (b"/x[^0-9]{2,3}y$/", [b"xaby", b"x1by", b"xabcdy", b"zzzzzzzzxaby", b"xabyz"]),     # negated class, {n,m}, $ at a_cap
    (b"/^\\.[abc]{2}/", [b".ab", b"xab", b".ad"]),                                       # escape, class list, {n}, ^ alone
    (b"/ba{2,}b/", [b"baab", b"bab", b"xbaaaaaaaab"]),                                   # {n,}
    (b"/ba{,2}b/", [b"bb", b"baab", b"baaab"]),                                          # {,m}
    (b"/abc$/", [b"xxabc", b"abcx"]),                                                    # a literal: the ends_with_clear plan
]


@pytest.mark.parametrize("pattern,strings", CASES, ids=[p.decode() for p, _ in CASES])
def test_matches_vs_re(rig, pattern, strings):
    P, ck, eng, ops = rig
    for s in strings:
        out = ops.matches(_enc(rig, s), pattern)
        assert out.shape == (P.big_size,)
        assert ck.decrypt(out.reshape(1, -1))[0] == has_match(s, pattern), (pattern, s)


def test_fhe_str_matches_clear_directly(rig):
    """The C entry point as a C caller uses it; refusals come back as errors with the reason."""
    import fhestr
    P, ck, eng, ops = rig
    L = fhestr.lib()
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    pattern = b"/^[a-c]+[0-9]{2}$/i"
    buf = (C.c_uint8 * len(pattern))(*pattern)
    for s in (b"Ab12", b"ab123", b"12"):
        a = np.ascontiguousarray(_enc(rig, s))
        out = np.zeros((1, P.big_size), dtype=np.uint64)
        assert L.fhe_str_matches_clear(eng.handle, ptr(a), A_CAP, buf, len(pattern), ptr(out)) == 0, L.fhe_last_error()
        assert ck.decrypt(out)[0] == has_match(s, pattern), s
    m, longest = C.c_uint32(0), C.c_uint32(0)
    assert L.fhe_regex_check(buf, len(pattern), C.byref(m), C.byref(longest)) == 0
    assert (m.value, longest.value) == (3, 0xFFFFFFFF)
    assert L.fhe_regex_check(buf, len(pattern), None, None) == 0
    bad = b"/a(b/"
    assert L.fhe_str_matches_clear(eng.handle, ptr(a), A_CAP, (C.c_uint8 * len(bad))(*bad), len(bad), ptr(out)) != 0
    assert b"malformed pattern at byte 4" in L.fhe_last_error()
    assert L.fhe_regex_check((C.c_uint8 * len(bad))(*bad), len(bad), C.byref(m), None) != 0
    assert b"malformed pattern at byte 4" in L.fhe_last_error()


def test_packed_operand_and_packed_result(rig):
    import fhestr
    P, ck, eng, ops = rig
    pattern = b"/[a-z]+@[a-z]+/"
    n_blocks = A_CAP * ops.bpc
    for s in (b"me@host", b"me@"):
        a = _enc(rig, s)
        packed_in = fhestr.PackedString(eng.pack(a), n_blocks, A_CAP)
        assert ck.decrypt(ops.matches(packed_in, pattern).reshape(1, -1))[0] == has_match(s, pattern)
        res = ops.matches(a, pattern, packed=True)
        assert isinstance(res, fhestr.PackedString)
        assert ck.decrypt_packed(res, 1)[0] == has_match(s, pattern)


def test_matches_many_equals_single_runs(rig):
    P, ck, eng, ops = rig
    pattern = b"/^[a-z]+(-[a-z]+)*$/"
    texts = [b"", b"a", b"ab-cd", b"ab--cd", b"abcdefghijkl", b"abcdefghijk-", b"-a", b"a-b-c-d-e-f"]
    rows = np.stack([_enc(rig, t) for t in texts])
    many = ops.matches_many(rows, pattern)
    assert many.shape == (8, P.big_size)
    got = ck.decrypt(many).tolist()
    assert got == [has_match(t, pattern) for t in texts]
    assert got == [int(ck.decrypt(ops.matches(rows[r], pattern).reshape(1, -1))[0]) for r in range(len(texts))]
    assert 0 in got and 1 in got


@pytest.mark.parametrize("p", [O.TOY_K1], ids=lambda p: p.name)
def test_matches_plans_run_bit_for_bit_on_the_exact_rig(p):
    """matches_clear is compared by its whole name, so the every-dispatch-name run of tests/test_gpu_exact_plan.py does not
    reach it: the same rig and the same check here -- a looped pattern, a bounded one with a wide class and /i, a nullable
    anchored one, a literal shortcut."""
    import test_gpu_exact_plan as exact
    with exact._rig(p) as rig:
        for pattern in (b"/a[bc]+d$/", b"/[^a]x|yz/i", b"/^(ab)*$/", b"/ab/"):
            name = "matches_clear " + pattern.decode()
            exact._check_run(rig, name, rig.string_op("matches_clear", 3, 0, pattern))
