"""repeat, replacen, splitn and rsplitn with an ENCRYPTED count, without a GPU: the C++ planner builds offline plans
on TOY_K1 (msg_mod = 4), the CPU oracle executes their exported levels, results are compared with the clear-text
definitions of tests/count_ref.py.

The count travels in D base-4 digits, D the smallest with 4^D > n_max.  Unless a test says otherwise n_max = 2, so
D = 1 and n runs over 0 .. 4^D - 1 = 3: n = 3 lies above the bound and must act as n = 2."""
import types

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from count_ref import encode_count, input_digits, repeat_ref, replacen_ref, splitn_ref
from plan_oracle import OracleBackend, run_with_oracle
from split_ref import count_digits, decode_split

A_CAP = 8
M = O.TOY_K1.msg_mod
N_MAX, D = 2, 1                      # the default bound and its digit count
ALL_N = range(M ** D)                # 0 .. 3
assert input_digits(M, N_MAX) == D and max(ALL_N) > N_MAX

# the strings of tests/test_split_cpu.py
COMMA_STRINGS = [b"", b"abc", b",a,b", b"a,b,", b"a,,b", b",,", b"a,b,c,d"]
OVERLAPS = [(b"aaaa", b"aa"), (b"aaa", b"aa"), (b"abababa", b"aa"), (b"aaaa", b"aba"), (b"aaa", b"aba"), (b"abababa", b"aba")]
SPLITS = ("splitn", "rsplitn")


def _params(p=O.TOY_K1):
    return to_fhestr_params(p)


_PLANS = {}


def _plan(op, a_cap, b_cap=0, clear=None, world=1, params=None):
    import fhestr
    key = (op, a_cap, b_cap, clear, world, (params or O.TOY_K1).name)
    if key not in _PLANS:
        _PLANS[key] = fhestr.Plan.string_op(None, op, a_cap, b_cap, clear, world, params=_params(params or O.TOY_K1))
    return _PLANS[key]


def _enc(ks, s, cap):
    import fhestr
    return ks.ck.encrypt_many(fhestr.string_to_blocks(_params(), s, cap))


def _enc_count(ks, n, n_max):
    return ks.ck.encrypt_many(np.array(encode_count(M, n, n_max), dtype=np.uint64))


def _run(ks, plan, operands, run=run_with_oracle):
    return ks.ck.decrypt_many(run(plan, np.concatenate(operands), ks.sk))


def _string(msgs):
    import fhestr
    return fhestr.blocks_to_string(_params(), msgs)


def _repeat(ks, s, n, n_max=N_MAX, a_cap=A_CAP):
    plan = _plan(f"repeat:{n_max}", a_cap)
    assert plan.info()["n_outputs"] == n_max * a_cap * 4
    return _string(_run(ks, plan, [_enc(ks, s, a_cap), _enc_count(ks, n, n_max)]))


def _splitn(ks, op, s, sep, n, max_parts=N_MAX, enc_cap=None, part_cap=None, world=1, run=run_with_oracle):
    """Decoded (count, parts); enc_cap: capacity of the encrypted pattern (None: clear pattern)."""
    name = f"{op}_encn" + ("_clear" if enc_cap is None else "") + f":{max_parts}" + (f":{part_cap}" if part_cap is not None else "")
    plan = _plan(name, A_CAP, enc_cap or 0, sep if enc_cap is None else None, world)
    operands = [_enc(ks, s, A_CAP)] + ([_enc(ks, sep, enc_cap)] if enc_cap else []) + [_enc_count(ks, n, max_parts)]
    return decode_split("splitn", _run(ks, plan, operands, run), M, max_parts, A_CAP if part_cap is None else part_cap)


def _replacen(ks, s, frm, to, n, n_max=N_MAX, enc_cap=None, out_cap=A_CAP):
    """enc_cap: capacity of each of the encrypted `from` and `to` (None: clear)."""
    if enc_cap is None:
        plan = _plan(f"replacen_encn_clear:{n_max}:{len(frm)}:{out_cap}", A_CAP, 0, frm + to)
        operands = [_enc(ks, s, A_CAP)]
    else:
        plan = _plan(f"replacen_encn:{n_max}:{enc_cap}:{out_cap}", A_CAP, 2 * enc_cap)
        operands = [_enc(ks, s, A_CAP), _enc(ks, frm, enc_cap), _enc(ks, to, enc_cap)]
    assert plan.info()["n_outputs"] == out_cap * 4
    return _string(_run(ks, plan, operands + [_enc_count(ks, n, n_max)]))


# ---- repeat -----------------------------------------------------------------------------------------------------------------

def test_repeat_every_count_offline_plan_vs_reference(toy_k1):
    """n = 0 gives the empty string, n = 3 > n_max = 2 acts as 2; a string that fills its capacity, a short and an empty one."""
    for s in (b"abcdefgh", b"ab", b"a,b,c,d", b""):
        for n in ALL_N:
            assert _repeat(toy_k1, s, n) == repeat_ref(s, n, N_MAX), (s, n)
    assert repeat_ref(b"ab", 3, N_MAX) == b"abab" and repeat_ref(b"ab", 0, N_MAX) == b""


# ---- splitn / rsplitn -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
@pytest.mark.parametrize("op", SPLITS)
def test_splitn_by_comma_offline_plan_vs_reference(toy_k1, op, encrypted):
    for s in COMMA_STRINGS:
        for n in ALL_N:
            got = _splitn(toy_k1, op, s, b",", n, enc_cap=1 if encrypted else None)
            assert got == splitn_ref(op, s, b",", n, N_MAX), (op, s, n, got)
    assert splitn_ref("splitn", b"a,b,c,d", b",", 0, 2) == (0, [b"", b""])
    assert splitn_ref("rsplitn", b"a,b,c,d", b",", 3, 2) == (2, [b"d", b"a,b,c"])


@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
@pytest.mark.parametrize("op", SPLITS)
def test_splitn_three_slots_offline_plan_vs_reference(toy_k1, op, encrypted):
    """n_max = P = 3 (D = 1, 3 is the largest value one digit holds): a middle slot takes the ordinary piece for n = 3 and
    the rest of the string for n = 2."""
    for s in (b"a,b,c,d", b",a,b", b"a,,b", b""):
        for n in range(4):
            got = _splitn(toy_k1, op, s, b",", n, max_parts=3, enc_cap=1 if encrypted else None)
            assert got == splitn_ref(op, s, b",", n, 3), (op, s, n, got)


@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
@pytest.mark.parametrize("op", SPLITS)
def test_splitn_self_overlapping_separator_offline_plan_vs_reference(toy_k1, op, encrypted):
    for s, sep in OVERLAPS:
        for n in ALL_N:
            got = _splitn(toy_k1, op, s, sep, n, enc_cap=len(sep) if encrypted else None)
            assert got == splitn_ref(op, s, sep, n, N_MAX), (op, s, sep, n, got)


@pytest.mark.parametrize("op", SPLITS)
def test_splitn_padded_empty_and_long_patterns(toy_k1, op):
    """An encrypted pattern of hidden length (capacity 4), one that decrypts to the empty string (separates nothing),
    and patterns longer than the string / than the capacity."""
    for n in ALL_N:
        for s, sep in ((b"a,b,c,d", b","), (b"xabyab", b"ab"), (b"ababab", b"ab")):
            assert _splitn(toy_k1, op, s, sep, n, enc_cap=4) == splitn_ref(op, s, sep, n, N_MAX), (op, s, sep, n)
        for s in (b"abc", b"", b"abcdefgh"):
            assert _splitn(toy_k1, op, s, b"", n, enc_cap=2) == splitn_ref(op, s, b"", n, N_MAX), (op, s, n)
        for sep, enc_cap in ((b"abcd", None), (b"abcd", 4), (b"abcdefghi", None)):
            assert _splitn(toy_k1, op, b"ab", sep, n, enc_cap=enc_cap) == splitn_ref(op, b"ab", sep, n, N_MAX), (op, sep, n)


@pytest.mark.parametrize("op", SPLITS)
def test_splitn_parts_are_cut_at_part_cap(toy_k1, op):
    for s in (b"abc,d,ef", b"a,bcdefg"):
        for enc_cap in (None, 1):
            for n in ALL_N:
                got = _splitn(toy_k1, op, s, b",", n, enc_cap=enc_cap, part_cap=2)
                assert got == splitn_ref(op, s, b",", n, N_MAX, part_cap=2), (op, s, enc_cap, n, got)


# ---- replacen ---------------------------------------------------------------------------------------------------------------

REPLACE_CASES = [(b"abcabc", b"bc", b"XY"), (b"aaaa", b"aa", b"bc"), (b"aaa", b"aa", b"xy"), (b"hello", b"zz", b"yy"),
                 (b"abababab", b"aba", b"xyz"), (b"", b"a", b"b"), (b"abcabc", b"b", b"XYZ"), (b"aaaa", b"aa", b"b"),
                 (b"hello", b"l", b""), (b"a,b,c,d", b",", b";"), (b"a,,b", b",", b""), (b",,", b",", b"ab")]


@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
def test_replacen_every_count_offline_plan_vs_reference(toy_k1, encrypted):
    """Encrypted `from` / `to` are zero padded to capacity 4 each (hidden lengths)."""
    for s, frm, to in REPLACE_CASES[:8] if encrypted else REPLACE_CASES:
        out_cap = max(A_CAP, len(s.replace(frm, to)))
        for n in ALL_N:
            got = _replacen(toy_k1, s, frm, to, n, enc_cap=4 if encrypted else None, out_cap=out_cap)
            assert got == replacen_ref(s, frm, to, n, N_MAX), (s, frm, to, n, got)
    assert replacen_ref(b"aaaa", b"a", b"b", 3, 2) == b"bbaa" and replacen_ref(b"aaaa", b"a", b"b", 0, 2) == b"aaaa"


def test_replacen_empty_and_long_encrypted_patterns_and_the_out_cap_cut(toy_k1):
    for n in ALL_N:
        for s in (b"abc", b""):                              # an empty encrypted `from` selects nothing
            assert _replacen(toy_k1, s, b"", b"xy", n, enc_cap=2) == replacen_ref(s, b"", b"xy", n, N_MAX)
        assert _replacen(toy_k1, b"ab", b"abcd", b"x", n, enc_cap=4) == b"ab"             # longer than the string
        assert _replacen(toy_k1, b"ab", b"abcdefghi", b"x", n) == b"ab"                   # longer than the capacity
        for enc_cap in (None, 3):                            # b"aXYZcaXYZcab" cut at 6 characters
            got = _replacen(toy_k1, b"abcabcab", b"b", b"XYZ", n, enc_cap=enc_cap, out_cap=6)
            assert got == replacen_ref(b"abcabcab", b"b", b"XYZ", n, N_MAX, out_cap=6), (enc_cap, n, got)


# ---- D = 2 ------------------------------------------------------------------------------------------------------------------

def test_two_digit_count_every_value(toy_k1):
    """n_max = 4 >= msg_mod: D = 2, the thermometer comes from the scalar comparison on the packed digit pair; every
    n from 0 to 4^2 - 1 = 15, all above 4 acting as 4."""
    assert input_digits(M, 4) == 2
    for n in range(M ** 2):
        assert _repeat(toy_k1, b"ab", n, n_max=4, a_cap=2) == repeat_ref(b"ab", n, 4), n
        for op in SPLITS:
            assert _splitn(toy_k1, op, b"a,b,c,d", b",", n, max_parts=4) == splitn_ref(op, b"a,b,c,d", b",", n, 4), (op, n)
        assert _replacen(toy_k1, b"aaaaaaa", b"a", b"X", n, n_max=4) == replacen_ref(b"aaaaaaa", b"a", b"X", n, 4), n
    assert _splitn(toy_k1, "splitn", b"a,b,c", b",", 9, max_parts=4, enc_cap=1) == (3, [b"a", b"b", b"c", b""])


def test_three_digit_count_takes_the_sign_tree(toy_k1):
    """n_max = 16: D = 3, two packed units, the most significant non-equal one wins."""
    assert input_digits(M, 16) == 3
    for n in (0, 1, 3, 4, 5, 15, 16, 17, 20, 32, 63):
        assert _replacen(toy_k1, b"aaaaaaaa", b"a", b"X", n, n_max=16) == replacen_ref(b"aaaaaaaa", b"a", b"X", n, 16), n


# ---- against the clear-count plans ------------------------------------------------------------------------------------------

def test_encrypted_count_equals_the_clear_count_plan(toy_k1):
    """For every n in 1 .. n_max the encrypted-count plan decrypts to what the clear-count plan of that n gives, the
    smaller layout padded to the larger one (parts that do not exist / characters past the end are zero)."""
    ks, n_max = toy_k1, 3
    for n in range(1, n_max + 1):
        s = b"ab,c,,d"
        clear_rep = _string(_run(ks, _plan("repeat_clear", 2, 0, bytes([n])), [_enc(ks, b"xy", 2)]))
        assert _repeat(ks, b"xy", n, n_max=n_max, a_cap=2) == clear_rep == b"xy" * n
        for op in SPLITS:
            for enc_cap in (None, 1):
                name = op + ("_clear" if enc_cap is None else "") + f":{n}"
                operands = [_enc(ks, s, A_CAP)] + ([_enc(ks, b",", 1)] if enc_cap else [])
                count, parts = decode_split(op, _run(ks, _plan(name, A_CAP, enc_cap or 0, b"," if enc_cap is None else None), operands), M, n, A_CAP)
                assert _splitn(ks, op, s, b",", n, max_parts=n_max, enc_cap=enc_cap) == (count, parts + [b""] * (n_max - n)), (op, n)
        for enc_cap in (None, 2):
            if enc_cap is None:
                clear_plan, operands = _plan(f"replacen_clear:{n}:1:10", A_CAP, 0, b",xy"), [_enc(ks, s, A_CAP)]
            else:
                clear_plan = _plan(f"replacen:{n}:2:10", A_CAP, 4)
                operands = [_enc(ks, s, A_CAP), _enc(ks, b",", 2), _enc(ks, b"xy", 2)]
            assert _replacen(ks, s, b",", b"xy", n, n_max=n_max, enc_cap=enc_cap, out_cap=10) == _string(_run(ks, clear_plan, operands)), n


def test_len_of_another_string_is_the_count_of_repeat(toy_k1):
    """Chaining: the digit ciphertexts `len` returns are the count operand as they are.  len of a capacity-8 string has
    two digits, so the bound is a two-digit one: n_max = 4 (a longer b repeats 4 times), and n_max = 4^2 - 1 = 15."""
    ks = toy_k1
    len_plan = _plan("len", A_CAP)
    assert len_plan.info()["n_outputs"] == 2 == input_digits(M, 4) == input_digits(M, 15)
    for b, n_max in ((b"abc", 4), (b"abcdef", 4), (b"", 4), (b"abcdefg", 15)):
        digits = run_with_oracle(len_plan, _enc(ks, b, A_CAP), ks.sk)
        got = _string(_run(ks, _plan(f"repeat:{n_max}", 2), [_enc(ks, b"xy", 2), digits]))
        assert got == b"xy" * min(len(b), n_max), (b, n_max, got)


# ---- refusals ---------------------------------------------------------------------------------------------------------------

REFUSALS = [   # (op, b_cap, clear, what fhe_last_error names)
    ("repeat", 0, None, "pattern capacity must be > 0"),
    ("repeat", 2, None, "repeat_clear takes one clear byte"),
    ("repeat:0", 0, None, "n_max must be in 1..255"),
    ("repeat:256", 0, None, "n_max must be in 1..255"),
    ("repeat:2:2", 0, None, "one parameter"),
    ("repeat:2", 2, None, "takes no second string"),
    ("splitn_encn:0", 1, None, "n must be at least 1"),
    ("rsplitn_encn_clear:0", 0, b",", "n must be at least 1"),
    ("splitn_encn_clear:2", 0, b"", "must not be empty"),
    ("splitn_encn", 1, None, "max_parts"),
    ("replacen_encn:0:1:8", 2, None, "n_max must be at least 1"),
    ("replacen_encn_clear:0:1:8", 0, b"ax", "n_max must be at least 1"),
    ("replacen_encn_clear:2:0:8", 0, b"x", "must not be empty"),
    ("replacen_encn_clear:2:8", 0, b"ax", "three parameters"),
]


@pytest.mark.parametrize("op,b_cap,clear,reason", REFUSALS)
def test_refusals_return_an_error_that_names_the_reason(op, b_cap, clear, reason):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        fhestr.Plan.string_op(None, op, A_CAP, b_cap, clear, params=_params())
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()


def test_the_digits_are_the_last_inputs_and_a_wrong_number_of_them_is_refused():
    """n_inputs = the string, the pattern operand(s), then exactly D digits; FheStringOps checks the digit ciphertexts it
    is given against the bound that travels with them before anything runs (no engine call is reached here)."""
    import fhestr
    for name, b_cap, clear, n_max in (("repeat:2", 0, None, 2), ("repeat:4", 0, None, 4), ("repeat:16", 0, None, 16),
                                      ("splitn_encn:3", 2, None, 3), ("rsplitn_encn_clear:4", 0, b",", 4),
                                      ("replacen_encn:16:1:8", 3, None, 16), ("replacen_encn_clear:2:1:8", 0, b"ab", 2)):
        assert _plan(name, A_CAP, b_cap, clear).info()["n_inputs"] == (A_CAP + b_cap) * 4 + input_digits(M, n_max), name
    p = _params()
    assert [fhestr.count_input_digits(p, n) for n in (1, 3, 4, 15, 16, 255)] == [1, 1, 2, 2, 3, 4]
    assert list(fhestr.encode_count(p, 9, 4)) == encode_count(M, 9, 4) == [1, 2]
    with pytest.raises(fhestr.FheError):
        fhestr.encode_count(p, 4, 3)                         # one digit does not hold 4
    with pytest.raises(fhestr.FheError):
        fhestr.EncryptedCount(np.zeros((1, p.big_size), dtype=np.uint64), 0)
    assert fhestr.EncryptedCount(np.zeros((2, p.big_size), dtype=np.uint64), params=p).n_max == 15
    ops = fhestr.FheStringOps(types.SimpleNamespace(params=p, device=0))
    a = np.zeros((A_CAP * 4, p.big_size), dtype=np.uint64)
    for digits, n_max in ((2, 2), (1, 4), (3, 15)):
        count = fhestr.EncryptedCount(np.zeros((digits, p.big_size), dtype=np.uint64), n_max)
        for call in (lambda: ops.repeat(a, count), lambda: ops.splitn(a, b",", count), lambda: ops.rsplitn(a, b",", count),
                     lambda: ops.replacen(a, b"a", b"b", count), lambda: ops.op_many(f"repeat:{n_max}", a[None], count=count)):
            with pytest.raises(fhestr.FheError, match="digits"):
                call()
    with pytest.raises(fhestr.FheError, match="only splitn and rsplitn"):
        ops.split(a, b",", fhestr.EncryptedCount(np.zeros((1, p.big_size), dtype=np.uint64), 2))


# ---- cost -------------------------------------------------------------------------------------------------------------------

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
SHARING = [   # (encrypted-count plan with n_max = 3, the clear-count plan of n, a_cap, b_cap, clear of n)
    ("repeat:3", lambda n: "repeat_clear", 8, 0, lambda n: bytes([n])),
    ("splitn_encn:3", lambda n: f"splitn:{n}", 32, 2, lambda n: None),
    ("splitn_encn_clear:3", lambda n: f"splitn_clear:{n}", 32, 0, lambda n: b","),
    ("rsplitn_encn:3", lambda n: f"rsplitn:{n}", 32, 2, lambda n: None),
    ("rsplitn_encn_clear:3", lambda n: f"rsplitn_clear:{n}", 32, 0, lambda n: b","),
    ("replacen_encn:3:2:32", lambda n: f"replacen:{n}:2:32", 32, 4, lambda n: None),
    ("replacen_encn_clear:3:1:32", lambda n: f"replacen_clear:{n}:1:32", 32, 0, lambda n: b"o0"),
]


@pytest.mark.parametrize("enc_name,clear_name,a_cap,b_cap,clear", SHARING, ids=[row[0] for row in SHARING])
def test_the_expensive_pieces_run_once_not_once_per_candidate_count(enc_name, clear_name, a_cap, b_cap, clear):
    """"Run every n and select" would cost the sum of the clear-count plans before selecting; the encrypted-count plan
    must be cheaper than that sum (it runs the shifters, concat and the occurrence scan once per output)."""
    enc_clear = clear(1) if enc_name != "repeat:3" else None
    enc = _plan(enc_name, a_cap, b_cap, enc_clear, params=P22).info()["n_pbs"]
    every_n = sum(_plan(clear_name(n), a_cap, b_cap, clear(n), params=P22).info()["n_pbs"] for n in (1, 2, 3))
    assert enc < every_n, (enc, every_n)


# PARAM_MESSAGE_2_CARRY_2, n_max = 4 (D = 2): (op, a_cap, b_cap, clear, n_pbs, n_levels) -- the figures of DESIGN.md section 3
P22_PINS = [("repeat:4", 8, 0, None, 1988, 22), ("splitn_encn:4", 32, 2, None, 5814, 52), ("splitn_encn_clear:4", 32, 0, b",", 5639, 23),
            ("rsplitn_encn_clear:4", 32, 0, b",", 5399, 20), ("replacen_encn:4:2:32", 32, 4, None, 9477, 72),
            ("replacen_encn_clear:4:1:32", 32, 0, b"o0", 715, 19)]


@pytest.mark.parametrize("op,a_cap,b_cap,clear,n_pbs,n_levels", P22_PINS, ids=[row[0] for row in P22_PINS])
def test_p22_plans_build_within_the_noise_budget_at_pinned_cost(op, a_cap, b_cap, clear, n_pbs, n_levels):
    plan = _plan(op, a_cap, b_cap, clear, params=P22)
    info, noise = plan.info(), plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]
    assert (info["n_pbs"], info["n_levels"]) == (n_pbs, n_levels)
    if "splitn" in op:
        assert info["n_outputs"] == count_digits(4, 4) + 4 * a_cap * 4      # the layout of splitn:4
    # the same names on TOY_K1, one- and two-digit counts
    for n_max in (3, 4):
        toy = _plan(op.replace(":4", f":{n_max}", 1), A_CAP, b_cap, clear).noise_info()
        assert toy["max_pbs_input_noise"] <= toy["budget"], (op, n_max)


# the clear-count plans keep their shape: (op, a_cap, b_cap, clear, n_pbs, n_levels) of the commit before
UNCHANGED_P22 = [("splitn_clear:4", 32, 0, b",", 5532, 23), ("splitn:4", 32, 2, None, 5707, 52), ("rsplitn_clear:4", 32, 0, b",", 5298, 20),
                 ("replacen_clear:2:1:32", 32, 0, b"o0", 450, 12), ("replacen:2:2:32", 32, 4, None, 9212, 67),
                 ("repeat_clear", 8, 0, b"\x04", 1856, 20)]


def test_clear_count_plans_are_unchanged():
    for op, a_cap, b_cap, clear, n_pbs, n_levels in UNCHANGED_P22:
        info = _plan(op, a_cap, b_cap, clear, params=P22).info()
        assert (info["n_pbs"], info["n_levels"]) == (n_pbs, n_levels), op


# ---- two ranks --------------------------------------------------------------------------------------------------------------

def _run_two_ranks(plan, inputs, sk):
    """Both ranks of a world-2 plan in one process: each runs only the jobs it owns into its own pool; what a level
    exports is copied where the all-gather would put it."""
    info = plan.info()
    assert info["world"] == 2
    backends = [OracleBackend(plan, sk) for _ in range(2)]
    pools = [b.alloc_pool(info["pool_slots"]) for b in backends]
    for b, pool in zip(backends, pools):
        b.load_inputs(pool, inputs, info["n_inputs"])
    for l in range(info["n_levels"]):
        lv = plan.level_info(l)
        for r in range(2):
            backends[r].run_level(pools[r], l, r)
        if lv["e_max"]:
            mine = [pools[r][lv["local_base"]: lv["local_base"] + lv["e_max"]].copy() for r in range(2)]
            for pool in pools:
                for r in range(2):
                    pool[lv["recv_base"] + r * lv["e_max"]: lv["recv_base"] + (r + 1) * lv["e_max"]] = mine[r]
    outs = [b.gather_outputs(pool, info["n_outputs"]) for b, pool in zip(backends, pools)]
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def test_world_2_build_decrypts_to_the_same_outputs(toy_k1):
    for n in ALL_N:
        single = _splitn(toy_k1, "splitn", b"ab,c,,d", b",", n, enc_cap=2)
        assert single == splitn_ref("splitn", b"ab,c,,d", b",", n, N_MAX)
        assert _splitn(toy_k1, "splitn", b"ab,c,,d", b",", n, enc_cap=2, world=2, run=_run_two_ranks) == single
