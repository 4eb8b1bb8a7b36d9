"""The split family and replacen without a GPU: the C++ planner builds offline plans on TOY_K1, the CPU
oracle executes their exported levels, results are compared with the clear-text definitions of
tests/split_ref.py (Rust's `str` methods stated with Python `bytes`)."""
import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from plan_oracle import OracleBackend, run_with_oracle
from split_ref import ONCE, SPLIT_OPS, decode_split, split_ref

A_CAP = 8
M = O.TOY_K1.msg_mod


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


def _name(op, clear, max_parts, part_cap=None):
    name = op + ("_clear" if clear else "")
    if op not in ONCE:
        name += f":{max_parts}"
    if part_cap is not None:
        name += f":{part_cap}"
    return name


def _split(ks, op, s, sep, max_parts, enc_cap=None, part_cap=None, world=1, run=run_with_oracle):
    """Decoded (count, parts) of the plan for `op`; enc_cap: capacity of the encrypted pattern (None: clear pattern)."""
    clear = enc_cap is None and sep is not None
    plan = _plan(_name(op, clear, max_parts, part_cap), A_CAP, enc_cap or 0, sep if clear else None, world)
    inputs = _enc(ks, s, A_CAP)
    if enc_cap:
        inputs = np.concatenate([inputs, _enc(ks, sep, enc_cap)])
    out = ks.ck.decrypt_many(run(plan, inputs, ks.sk))
    return decode_split(op, out, M, max_parts, A_CAP if part_cap is None else part_cap)


COMMA_STRINGS = [b"", b"abc", b",a,b", b"a,b,", b"a,,b", b",,", b"a,b,c,d"]
# where the leftmost-first and the rightmost-first selection differ (self-overlapping separators)
OVERLAPS = [(b"aaaa", b"aa"), (b"aaa", b"aa"), (b"abababa", b"aa"), (b"aaaa", b"aba"), (b"aaa", b"aba"), (b"abababa", b"aba")]


@pytest.mark.parametrize("max_parts", [2, 3])
@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_by_comma_offline_plan_vs_reference(toy_k1, op, encrypted, max_parts):
    """More parts than max_parts occur (b"a,b,c,d"), so count == max_parts + 1 is met; empty first, middle and last parts."""
    for s in COMMA_STRINGS:
        got = _split(toy_k1, op, s, b",", max_parts, enc_cap=1 if encrypted else None)
        assert got == split_ref(op, s, b",", max_parts), (op, s, got)


@pytest.mark.parametrize("max_parts", [2, 3])
@pytest.mark.parametrize("encrypted", [False, True], ids=["clear", "encrypted"])
@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_self_overlapping_separator_offline_plan_vs_reference(toy_k1, op, encrypted, max_parts):
    """b"aaa" by b"aa": split cuts ["", "a"] after the first two characters, rsplit before the last two."""
    for s, sep in OVERLAPS:
        got = _split(toy_k1, op, s, sep, max_parts, enc_cap=len(sep) if encrypted else None)
        assert got == split_ref(op, s, sep, max_parts), (op, s, sep, got)
    assert split_ref("split", b"aaa", b"aa", 2)[1] == split_ref("rsplit", b"aaa", b"aa", 2)[1] == [b"", b"a"]
    assert split_ref("split_inclusive", b"abababa", b"aba", 3)[1] == [b"aba", b"baba", b""]


@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_separator_longer_than_the_string(toy_k1, op):
    for sep, enc_cap in ((b"abcd", None), (b"abcd", 4), (b"abcdefghi", None)):       # the last one: longer than the capacity
        got = _split(toy_k1, op, b"ab", sep, 2, enc_cap=enc_cap)
        assert got == split_ref(op, b"ab", sep, 2), (op, sep, enc_cap, got)


@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_parts_are_cut_at_part_cap(toy_k1, op):
    for s in (b"abc,d,ef", b"a,bcdefg"):
        for enc_cap in (None, 1):
            got = _split(toy_k1, op, s, b",", 2, enc_cap=enc_cap, part_cap=2)
            assert got == split_ref(op, s, b",", 2, part_cap=2), (op, s, enc_cap, got)


@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_padded_encrypted_pattern(toy_k1, op):
    """A pattern of hidden length: b"," and b"ab" in capacity 4."""
    for s, sep in ((b"a,b,c,d", b","), (b",a,b", b","), (b"xabyab", b"ab"), (b"ababab", b"ab"), (b"abxab", b"ab")):
        got = _split(toy_k1, op, s, sep, 3, enc_cap=4)
        assert got == split_ref(op, s, sep, 3), (op, s, sep, got)


@pytest.mark.parametrize("op", SPLIT_OPS)
def test_split_empty_encrypted_pattern_separates_nothing(toy_k1, op):
    """The convention of replace (include/fhestr.h), a deviation from Rust: as with a separator that does not occur."""
    for s in (b"abc", b"", b"abcdefgh"):
        got = _split(toy_k1, op, s, b"", 2, enc_cap=2)
        assert got == split_ref(op, s, b"\xff", 2), (op, s, got)


@pytest.mark.parametrize("s", [b"  a b ", b"\ta\n\nb", b"    ", b"ab", b"", b"a b c d", b"a\x0bb\x0c\rc"])
def test_split_ascii_whitespace_offline_plan_vs_reference(toy_k1, s):
    """Whitespace = ASCII 9..13 and 32 (0x0B included, as trim_* and Python's bytes.split())."""
    for max_parts, part_cap in ((2, None), (3, None), (1, None), (3, 2)):
        got = _split(toy_k1, "split_ascii_whitespace", s, None, max_parts, part_cap=part_cap)
        assert got == split_ref("split_ascii_whitespace", s, None, max_parts, part_cap=part_cap), (s, max_parts, got)


def test_splitn_one_returns_the_string_and_large_max_parts_counts_in_two_digits(toy_k1):
    for op in ("splitn", "rsplitn"):
        assert _split(toy_k1, op, b"a,b,c", b",", 1) == (1, [b"a,b,c"])
        assert _split(toy_k1, op, b"", b",", 1) == (1, [b""])
    # max_parts = 5: the count 6 needs two base-4 digits
    for s in (b"a,b,c,d", b"a,b,c,d,", b",,,,,,,", b"abc"):
        assert _split(toy_k1, "split", s, b",", 5) == split_ref("split", s, b",", 5)
        assert _split(toy_k1, "split_terminator", s, b",", 5) == split_ref("split_terminator", s, b",", 5)


# the replace cases of tests/test_strings_cpu.py: the equal-length ones, then the general ones
REPLACE_CASES = [(b"abcabc", b"bc", b"XY"), (b"aaaa", b"aa", b"bc"), (b"aaa", b"aa", b"xy"), (b"hello", b"zz", b"yy"),
                 (b"abababab", b"aba", b"xyz"), (b"", b"a", b"b"),
                 (b"abcabc", b"bc", b"X"), (b"abcabc", b"b", b"XYZ"), (b"aaaa", b"aa", b"b"), (b"aaa", b"aa", b"xyz"),
                 (b"hello", b"l", b""), (b"hello", b"zz", b"y"), (b"abab", b"ab", b"ab"), (b"", b"a", b"bc"), (b"abc", b"abc", b"z"),
                 (b"abcabc", b"abc", b"abcd")]


@pytest.mark.parametrize("n", [0, 1, 2, 5])
@pytest.mark.parametrize("s,frm,to", REPLACE_CASES)
def test_replacen_clear_offline_plan_vs_python(toy_k1, s, frm, to, n):
    import fhestr
    want = s.replace(frm, to, n)
    out_cap = max(A_CAP, len(want))
    plan = _plan(f"replacen_clear:{n}:{len(frm)}:{out_cap}", A_CAP, 0, frm + to)
    got = fhestr.blocks_to_string(_params(), toy_k1.ck.decrypt_many(run_with_oracle(plan, _enc(toy_k1, s, A_CAP), toy_k1.sk)))
    assert got == want
    assert plan.info()["n_outputs"] == out_cap * 4


@pytest.mark.parametrize("n", [0, 1, 2, 5])
@pytest.mark.parametrize("s,frm,to", REPLACE_CASES)
def test_replacen_encrypted_padded_offline_plan_vs_python(toy_k1, s, frm, to, n):
    """Encrypted `from` / `to` of hidden lengths (capacity 4 each), as the general replace takes them."""
    import fhestr
    want = s.replace(frm, to, n)
    out_cap = max(A_CAP, len(want))
    plan = _plan(f"replacen:{n}:4:{out_cap}", A_CAP, 8)
    inputs = np.concatenate([_enc(toy_k1, s, A_CAP), _enc(toy_k1, frm, 4), _enc(toy_k1, to, 4)])
    got = fhestr.blocks_to_string(_params(), toy_k1.ck.decrypt_many(run_with_oracle(plan, inputs, toy_k1.sk)))
    assert got == want


def test_replacen_cuts_at_out_cap(toy_k1):
    import fhestr
    plan = _plan("replacen_clear:2:1:6", A_CAP, 0, b"bXYZ")
    got = fhestr.blocks_to_string(_params(), toy_k1.ck.decrypt_many(run_with_oracle(plan, _enc(toy_k1, b"abcabcab", A_CAP), toy_k1.sk)))
    assert got == b"abcabcab".replace(b"b", b"XYZ", 2)[:6]


REFUSALS = [   # (op, b_cap, clear, what fhe_last_error names)
    ("split_clear:2", 0, b"", "must not be empty"),
    ("rsplit_once_clear", 0, b"", "must not be empty"),
    ("split:0", 4, None, "max_parts must be at least 1"),
    ("split_inclusive_clear:0", 0, b",", "max_parts must be at least 1"),
    ("split_ascii_whitespace:0", 0, None, "max_parts must be at least 1"),
    ("splitn:0", 4, None, "n must be at least 1"),
    ("rsplitn_clear:0", 0, b",", "n must be at least 1"),
    ("split_clear:2:0", 0, b",", "part capacity must be > 0"),
    ("split_once:0", 4, None, "part capacity must be > 0"),
    ("split_ascii_whitespace:2", 0, b" ", "takes no pattern"),
    ("split_ascii_whitespace_clear:2", 0, b" ", "takes no pattern"),
    ("split_clear", 0, b",", "max_parts"),
    ("split", 0, None, "pattern capacity must be > 0"),
    ("replacen_clear:1:0:8", 0, b"x", "must not be empty"),
    ("replacen_clear:1:8", 0, b"ax", "three parameters"),
]


@pytest.mark.parametrize("op,b_cap,clear,reason", REFUSALS)
def test_refusals_return_an_error_that_names_the_reason(op, b_cap, clear, reason):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        fhestr.Plan.string_op(None, op, A_CAP, b_cap, clear, params=_params())
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()


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


@pytest.mark.parametrize("op,s,sep,max_parts,enc_cap", [("split", b"a,b,,c", b",", 3, None), ("rsplitn", b"abxabyab", b"ab", 2, 4)])
def test_world_2_build_decrypts_to_the_same_outputs(toy_k1, op, s, sep, max_parts, enc_cap):
    single = _split(toy_k1, op, s, sep, max_parts, enc_cap=enc_cap)
    assert single == split_ref(op, s, sep, max_parts)
    sharded = _split(toy_k1, op, s, sep, max_parts, enc_cap=enc_cap, world=2,
                     run=lambda plan, inputs, sk: _run_two_ranks(plan, inputs, sk))
    assert sharded == single
    plan = _plan(_name(op, enc_cap is None, max_parts), A_CAP, enc_cap or 0, sep if enc_cap is None else None, 2)
    jobs = [sum(plan.level_rank_info(l, r)["job_hi"] - plan.level_rank_info(l, r)["job_lo"] for l in range(plan.info()["n_levels"]))
            for r in range(2)]
    assert min(jobs) * 3 >= max(jobs), jobs          # both ranks carry a real share of the lookups


# (op, a_cap, b_cap, clear) -> (n_pbs, n_levels) of the commit before these operations were added
UNCHANGED_TOY = [
    ("replace_clear", 8, 0, b"bcXY", 67, 3), ("replace", 8, 4, None, 131, 6), ("replace:2:8", 8, 4, None, 1119, 23),
    ("replace_clear:2:9", 8, 0, b"bcXYZ", 1498, 15), ("trim_start", 8, 0, None, 215, 8), ("find", 8, 4, None, 94, 6),
    ("find_clear", 8, 0, b"ab", 49, 5),
]
UNCHANGED_P22 = [
    ("trim_start", 32, 0, None, 1223, 11), ("trim_start", 64, 0, None, 2791, 13), ("find", 32, 4, None, 413, 7),
    ("replace:4:32", 32, 8, None, 21840, 67), ("replace_clear:1:32", 32, 0, b"o0", 224, 3),
]


@pytest.mark.parametrize("params,cases", [(O.TOY_K1, UNCHANGED_TOY), (O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, UNCHANGED_P22)],
                         ids=["toy_k1", "p22"])
def test_existing_operations_build_the_same_plans(params, cases):
    for op, a_cap, b_cap, clear, n_pbs, n_levels in cases:
        info = _plan(op, a_cap, b_cap, clear, params=params).info()
        assert (info["n_pbs"], info["n_levels"]) == (n_pbs, n_levels), op


# PARAM_MESSAGE_2_CARRY_2: (op, a_cap, b_cap, clear, n_pbs, n_levels), the figures of DESIGN.md section 3
P22_BUILDS = [("split_clear:4", 32, 0, b" ", 5510, 23), ("split:4", 32, 4, None, 5928, 53), ("split_clear:8", 64, 0, b",", 24630, 38)]


@pytest.mark.parametrize("op,a_cap,b_cap,clear,n_pbs,n_levels", P22_BUILDS)
def test_p22_split_plans_build_within_the_noise_budget(op, a_cap, b_cap, clear, n_pbs, n_levels):
    """About max_parts shifts of trim_start's size (1,223 PBS at 32 characters, 2,791 at 64) plus the occurrence
    bookkeeping: less than twice that."""
    plan = _plan(op, a_cap, b_cap, clear, params=O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    info, noise = plan.info(), plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]
    assert (info["n_pbs"], info["n_levels"]) == (n_pbs, n_levels)
    max_parts = int(op.split(":")[1])
    assert info["n_pbs"] < 2 * max_parts * (1223 if a_cap == 32 else 2791)
    assert info["n_outputs"] == 2 + max_parts * a_cap * 4      # max_parts + 1 in two base-4 digits


@pytest.mark.parametrize("params", [O.PARAM_MESSAGE_4_CARRY_4_KS_PBS, O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS],
                         ids=["p44", "p22_multibit_g2"])
def test_every_operation_builds_on_other_parameter_sets(params):
    """4-bit blocks (whole characters as lookup inputs), and the tightest budget among the 2-bit sets (grouping factor 2:
    split_inclusive and a long count take their low-noise forms there)."""
    for op in SPLIT_OPS:
        for name, b_cap, clear in ((_name(op, False, 3), 4, None), (_name(op, True, 3), 0, b"aba")):
            noise = _plan(name, 32, b_cap, clear, params=params).noise_info()
            assert noise["max_pbs_input_noise"] <= noise["budget"], name
    for name, b_cap, clear in (("split_ascii_whitespace:4", 0, None), ("split_clear:20", 0, b","), ("replacen_clear:1:1:32", 0, b"o0"),
                               ("replacen:2:4:32", 8, None)):
        noise = _plan(name, 32, b_cap, clear, params=params).noise_info()
        assert noise["max_pbs_input_noise"] <= noise["budget"], name


LONG_SEP_CAP = 15


@pytest.mark.parametrize("op", ["rsplit", "rsplitn", "rsplit_once"])
def test_right_to_left_split_by_a_long_clear_separator(toy_k1, op):
    """Regression, found by tests/test_plan_sweep_cpu.py: at 15 characters and more a clear separator of 6 characters and
    more was refused for rsplit, rsplitn and rsplit_once (106 .. 122 nominal variances against TOY_K1's 99.6; from 7
    characters on against PARAM_MESSAGE_2_CARRY_2's 138.2 as well).  A selection taken from the right rebuilds cover[i] as a
    sum of up to 8 selection bits, the part masks `nz - cover` went unrefreshed into prefix_or, and a run of 16 of them
    shares those bits: the run's noise as built is far above the 16 x 9 its terms add up to one by one.  prefix_or now gives
    the bits of such a run a lookup of their own first.  The separators have no border and a border; one occurrence, two,
    and none."""
    import fhestr
    from clear_plan import ClearBackend, run_clear
    for sep in (b"ab, xy", b"aab,aa", b"ab, xyz"):
        name = _name(op, True, 2)
        plan = _plan(name, LONG_SEP_CAP, 0, sep)
        assert plan.noise_info()["max_pbs_input_noise"] <= plan.noise_info()["budget"]
        for s in (sep, b"x" + sep + b"yz" + sep[:5], sep + sep + b"q", b"ab, xab, x", b""):
            s = s[:LONG_SEP_CAP]
            out = toy_k1.ck.decrypt_many(run_with_oracle(plan, _enc(toy_k1, s, LONG_SEP_CAP), toy_k1.sk))
            assert decode_split(op, out, M, 2, LONG_SEP_CAP) == split_ref(op, s, sep, 2), (op, s, sep)
        p22 = _plan(name, LONG_SEP_CAP, 0, sep, params=O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
        assert p22.noise_info()["max_pbs_input_noise"] <= p22.noise_info()["budget"]
        backend = ClearBackend(p22, _params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS))
        s = b"x" + sep + b"yz" + sep[:5]
        out = run_clear(backend, fhestr.string_to_blocks(_params(), s, LONG_SEP_CAP))
        assert decode_split(op, out, M, 2, LONG_SEP_CAP) == split_ref(op, s, sep, 2) and backend.off_centre == 0
