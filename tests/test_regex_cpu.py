"""matches (a clear regular expression against an encrypted string) without a GPU: the C++ planner builds offline plans
on TOY_K1, the CPU oracle executes their exported levels, results are compared with Python's `re` through the
translation of tests/regex_ref.py.  The reference's own 30 `has_match` rows are tests/golden/regex_has_match_cases.json."""
import json
import os

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from plan_oracle import OracleBackend, run_with_oracle
from regex_ref import has_match, random_pattern

A_CAP = 8
P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regex_has_match_cases.json")


def _params(p=O.TOY_K1):
    return to_fhestr_params(p)


_PLANS = {}


def _plan(op, a_cap, b_cap=0, clear=None, world=1, params=None):
    import fhestr
    key = (op, a_cap, b_cap, clear, world, (params or O.TOY_K1).name)
    if key not in _PLANS:
        _PLANS[key] = fhestr.Plan.string_op(None, op, a_cap, b_cap, clear, world, params=_params(params or O.TOY_K1))
    return _PLANS[key]


def _matches(ks, s, pattern, cap=A_CAP, world=1, run=run_with_oracle):
    import fhestr
    plan = _plan("matches_clear", cap, 0, pattern, world)
    out = ks.ck.decrypt_many(run(plan, ks.ck.encrypt_many(fhestr.string_to_blocks(_params(), s, cap)), ks.sk))
    assert out.shape == (1,)
    return int(out[0])


def test_reference_rows_agree_with_the_translation_and_the_plan(toy_k1):
    rows = json.load(open(GOLDEN))
    assert len(rows) == 30
    for row in rows:
        s, pattern = row["content"].encode(), row["pattern"].encode()
        assert has_match(s, pattern) == row["expected"], row
        assert _matches(toy_k1, s, pattern, cap=16) == row["expected"], row


# one pattern (at least) per construct: (pattern, strings beyond the common ones)
CONSTRUCTS = [
    (b"/bc/", [b"bcaaaaaa", b"aaaaaabc", b"abdc"]),                          # literal
    (b"/a.c/", [b"abcxxxxx", b"xxxxxabc", b"ac", b"a\nc"]),                   # any character
    (b"/a\\.c/", [b"a.cxxxxx", b"xxxxxa.c", b"abc"]),                        # escape
    (b"/x[abc]y/", [b"xbyzzzzz", b"zzzzzxcy", b"xdy"]),                      # class list
    (b"/[b-d]{2}/", [b"bdaaaaaa", b"aaaaaacc", b"abeb"]),                    # range, {n}
    (b"/a[^ab]/", [b"acbbbbbb", b"bbbbbba-", b"aab", b"a"]),                 # negated class
    (b"/ab?c/", [b"acxxxxxx", b"xxxxxabc", b"abbc"]),                        # ?
    (b"/ab*c/", [b"abbbbbbc", b"acxxxxxx", b"xxxxxxac", b"abbbbbbb"]),       # *
    (b"/ab+c/", [b"abcxxxxx", b"xxxxabbc", b"acac"]),                        # +
    (b"/ba{2,}b/", [b"baabxxxx", b"xxbaaaab", b"babab"]),                    # {n,}
    (b"/ba{,2}b/", [b"bbxxxxxx", b"xxxxbaab", b"baaab"]),                    # {,m}
    (b"/ba{1,2}b/", [b"babxxxxx", b"xxxxbaab", b"bb", b"baaab"]),            # {n,m}
    (b"/(ab|c)+d/", [b"abcabdxx", b"xxxxxxcd", b"abad"]),                    # group
    (b"/ab|cd|ef/", [b"efxxxxxx", b"xxxxxxcd", b"aceb"]),                    # alternation of three
    (b"/^ab|cd/", [b"cdxxxxxx", b"xcd", b"ab"]),                             # ^ alone
    (b"/ab|cd$/", [b"xxxxxxcd", b"cdx", b"ab"]),                             # $ alone
    (b"/^a+b?$/", [b"aaaaaaab", b"a", b"aaaaaaaa", b"aabb", b"ba"]),         # both anchors
    (b"/^(ab)*$/", [b"abababab", b"ab", b"aba"]),                            # both anchors, nullable: the empty string matches
    (b"/b+$/", [b"abbbbbbb", b"ab", b"ba"]),                                 # $ at the hidden end and at a_cap
    (b"/Ab/i", [b"aBxxxxxx", b"xxxxxxAB", b"a-b"]),                          # /i on a literal
    (b"/x[b-d]/i", [b"XCxxxxxx", b"ababaaxD", b"xa", b"XE"]),                # /i on a range
]
COMMON = [b"", b"abcdabcd", b"abababab"]          # the empty string, two of exactly A_CAP characters


@pytest.mark.parametrize("pattern,strings", CONSTRUCTS, ids=[p.decode() for p, _ in CONSTRUCTS])
def test_construct_offline_plan_vs_re(toy_k1, pattern, strings):
    """Per pattern: the empty string, strings of exactly a_cap characters, a match touching position 0, a match touching
    the hidden end, a near miss."""
    wanted = set()
    for s in COMMON + strings:
        assert len(s) <= A_CAP
        want = has_match(s, pattern)
        wanted.add(want)
        assert _matches(toy_k1, s, pattern) == want, (pattern, s)
    assert wanted == {0, 1}, pattern                  # both answers occur for every pattern


def test_deviations_from_the_reference_executor(toy_k1):
    assert _matches(toy_k1, b"aaa", b"/^a{,2}$/") == 0           # 1. repeat counts mean what they say
    assert _matches(toy_k1, b"aa", b"/^a{,2}$/") == 1
    assert _matches(toy_k1, b"B", b"/[a-c]/i") == 1              # 2. /i folds class members and range ends
    assert _matches(toy_k1, b"B", b"/[abc]/i") == 1
    assert _matches(toy_k1, b"B", b"/[a-c]/") == 0
    assert _matches(toy_k1, b"", b"/./") == 0                    # 4. a character never matches padding
    assert _matches(toy_k1, b"a", b"/[^a]/") == 0
    assert _matches(toy_k1, b"ab", b"/[^a]/") == 1
    assert _matches(toy_k1, b"ab", b"/^a.$/") == 1 and _matches(toy_k1, b"a", b"/^a.$/") == 0


def test_random_patterns_vs_re(toy_k1):
    """A fixed-seed batch: patterns of at most 6 positions, strings over {a, b, c} of every length up to a_cap."""
    import fhestr
    rng = np.random.default_rng(0x5EED)
    seen = set()
    for _ in range(40):
        pattern = random_pattern(rng, 6)
        info = fhestr.regex_check(pattern)
        assert info["positions"] <= 6, pattern
        for length in (0, 3, 6, A_CAP, int(rng.integers(1, A_CAP))):
            s = bytes(rng.choice(list(b"abc"), size=length).tolist())
            want = has_match(s, pattern)
            seen.add(want)
            assert _matches(toy_k1, s, pattern) == want, (pattern, s)
    assert seen == {0, 1}


def test_nullable_pattern_without_both_anchors_is_the_constant_one(toy_k1):
    for pattern in (b"/a*/", b"/^a?/", b"/(ab)*$/", b"/^/", b"/$/"):
        info = _plan("matches_clear", A_CAP, 0, pattern).info()
        assert (info["n_pbs"], info["n_levels"]) == (0, 0), pattern
        for s in (b"", b"xyz", b"abababab"):
            assert _matches(toy_k1, s, pattern) == 1 == has_match(s, pattern)
    for s, want in ((b"", 1), (b"a", 0), (b"abababab", 0)):
        assert _matches(toy_k1, s, b"/^$/") == want


LITERALS = [(b"/abc/", "contains_clear"), (b"/^abc/", "starts_with_clear"), (b"/abc$/", "ends_with_clear"), (b"/^abc$/", "eq_clear"),
            (b"/a\\.c/", "contains_clear")]


@pytest.mark.parametrize("a_cap", [16, 64])
@pytest.mark.parametrize("pattern,op", LITERALS, ids=[p.decode() for p, _ in LITERALS])
def test_plain_literal_builds_the_existing_plan(pattern, op, a_cap):
    literal = b"a.c" if b"\\" in pattern else b"abc"
    got = _plan("matches_clear", a_cap, 0, pattern, params=P22).info()
    want = _plan(op, a_cap, 0, literal, params=P22).info()
    assert got == want
    assert got["n_pbs"] > 0


def test_literal_shortcuts_decrypt_like_re(toy_k1):
    for pattern, _ in LITERALS:
        for s in (b"", b"abc", b"xabc", b"abcx", b"xxxxxabc", b"abcxxxxx", b"a.c", b"ab"):
            assert _matches(toy_k1, s, pattern) == has_match(s, pattern), (pattern, s)


@pytest.mark.parametrize("pattern", [b"/[a-z]{2}[0-9]/", b"/^[a-z]{2}[0-9]?$/", b"/(ab|cd).e/i"])
def test_bounded_pattern_depth_follows_the_pattern_not_the_capacity(pattern):
    """Without * + {n,} the follow graph has no cycle: the levels of all text positions coincide, and only the final OR
    over the positions grows with the capacity -- as contains_clear's does."""
    import fhestr
    assert fhestr.regex_check(pattern)["max_len"] is not None
    own = [_plan("matches_clear", cap, 0, pattern, params=P22).info()["n_levels"] for cap in (16, 64)]
    ref = [_plan("contains_clear", cap, 0, b"ab", params=P22).info()["n_levels"] for cap in (16, 64)]
    assert 0 <= own[1] - own[0] <= ref[1] - ref[0], (own, ref)


# PARAM_MESSAGE_2_CARRY_2: (pattern, a_cap, n_pbs, n_levels), the figures of DESIGN.md section 3
P22_PINS = [(b"/^[0-9]*$/", 32, 194, 35), (b"/[a-z]+@[a-z]+/", 32, 253, 35), (b"/ab|cd/i", 64, 707, 5)]


@pytest.mark.parametrize("pattern,a_cap,n_pbs,n_levels", P22_PINS, ids=[p.decode() for p, _, _, _ in P22_PINS])
def test_p22_plans_build_within_the_noise_budget(pattern, a_cap, n_pbs, n_levels):
    plan = _plan("matches_clear", a_cap, 0, pattern, params=P22)
    info, noise = plan.info(), plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]
    assert (info["n_pbs"], info["n_levels"]) == (n_pbs, n_levels)
    assert info["n_outputs"] == 1


def test_unbounded_pattern_depth_grows_with_the_capacity():
    import fhestr
    assert fhestr.regex_check(b"/^[0-9]*$/") == {"positions": 1, "max_len": None}
    levels = [_plan("matches_clear", cap, 0, b"/^[0-9]*$/", params=P22).info()["n_levels"] for cap in (8, 16, 32)]
    assert levels[0] < levels[1] < levels[2], levels


def test_every_p22_build_stays_inside_the_noise_budget():
    """Wide fan-in (seven alternatives into one position), classes of many rows, nested repeats."""
    for pattern in (b"/(a|b|c|d|e|f|g)+h$/", b"/(a|b|c|d|e|f|g|h|i|j)k/", b"/[adgjmpsvy0369]+x/i", b"/^(.[^a]){2,5}$/",
                    b"/(ab?|c*d){3}e{2,4}/", b"/[^0-9]+@.+\\..{2,3}$/"):
        for cap in (12, 32):
            noise = _plan("matches_clear", cap, 0, pattern, params=P22).noise_info()
            assert noise["max_pbs_input_noise"] <= noise["budget"], (pattern, cap)


REFUSALS = [   # (pattern, a_cap, what fhe_last_error names)
    (b"/ab", A_CAP, "malformed pattern at byte 3"),
    (b"ab/", A_CAP, "malformed pattern at byte 0"),
    (b"/a**/", A_CAP, "malformed pattern at byte 3"),
    (b"/a(b/", A_CAP, "malformed pattern at byte 4"),
    (b"/[a-]/", A_CAP, "malformed pattern at byte 3"),
    (b"/a/g", A_CAP, "malformed pattern at byte 3"),
    (b"//", A_CAP, "empty pattern"),
    (b"/a||b/", A_CAP, "empty alternative"),
    (b"/a()/", A_CAP, "empty group"),
    (b"/a{}/", A_CAP, "empty repeat count"),
    (b"/a{3,2}/", A_CAP, "n > m"),
    (b"/caf\xc3\xa9/", A_CAP, "non-ASCII byte at offset 4"),
    (b"/a{257}/", A_CAP, "more than 256 automaton positions"),
    (b"/(a{16}){17}/", A_CAP, "more than 256 automaton positions"),
    (b"/a{999999999}/", A_CAP, "more than 256 automaton positions"),
    (b"/ab/", 0, "capacity must be > 0"),
]


@pytest.mark.parametrize("pattern,a_cap,reason", REFUSALS, ids=[repr(p)[2:-1] + f"@{c}" for p, c, _ in REFUSALS])
def test_refusals_return_an_error_that_names_the_reason(pattern, a_cap, reason):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        fhestr.Plan.string_op(None, "matches_clear", a_cap, 0, pattern, params=_params())
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()
    if a_cap:
        with pytest.raises(fhestr.FheError) as err:
            fhestr.regex_check(pattern)
        assert reason in str(err.value), str(err.value)


def test_the_encrypted_form_and_parameters_are_refused():
    import fhestr
    for op, b_cap, clear, reason in (("matches", 4, None, "clear pattern"), ("matches", 0, None, "clear pattern"),
                                     ("matches_clear:2", 0, b"/a/", "no parameters"),
                                     ("matches_reference_clear", 0, b"/a/", "unknown string op"), ("matches_reference", 4, None, "unknown string op")):
        with pytest.raises(fhestr.FheError) as err:
            fhestr.Plan.string_op(None, op, A_CAP, b_cap, clear, params=_params())
        assert reason in str(err.value), str(err.value)


def test_256_positions_build_and_regex_check_reports_them():
    import fhestr
    assert fhestr.regex_check(b"/(a{16}){16}/") == {"positions": 256, "max_len": 256}
    assert fhestr.regex_check("/a{2,4}(b|cd)?/") == {"positions": 7, "max_len": 6}
    assert fhestr.regex_check(b"/a{0}/") == {"positions": 0, "max_len": 0}
    assert _plan("matches_clear", 4, 0, b"/(a{16}){16}/").info()["n_outputs"] == 1


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


@pytest.mark.parametrize("pattern", [b"/a[bc]+d$/", b"/^(ab|c)*$/", b"/b.d/i"])
def test_world_2_build_decrypts_to_the_same_answers(toy_k1, pattern):
    for s in (b"", b"abcd", b"xxabcbcd", b"abccabcc", b"abcabcab", b"aBxD"):
        single = _matches(toy_k1, s, pattern)
        assert single == has_match(s, pattern), (pattern, s)
        assert _matches(toy_k1, s, pattern, world=2, run=_run_two_ranks) == single, (pattern, s)
    plan = _plan("matches_clear", A_CAP, 0, pattern, 2)
    jobs = [sum(plan.level_rank_info(l, r)["job_hi"] - plan.level_rank_info(l, r)["job_lo"] for l in range(plan.info()["n_levels"]))
            for r in range(2)]
    assert min(jobs) * 3 >= max(jobs), jobs          # both ranks carry a real share of the lookups


@pytest.mark.parametrize("params", [O.PARAM_MESSAGE_4_CARRY_4_KS_PBS, O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS],
                         ids=["p44", "p22_multibit_g2"])
def test_matches_builds_on_other_parameter_sets(params):
    """4-bit blocks (a whole character is one lookup input: one lookup per class and character), and the tightest budget
    among the 2-bit sets."""
    for pattern in (b"/^[0-9]*$/", b"/[a-z]+@[a-z]+/", b"/ab|cd/i", b"/(a|b|c|d|e|f|g)+h$/", b"/[^a]{2,3}x/", b"/abc/"):
        plan = _plan("matches_clear", 32, 0, pattern, params=params)
        noise = plan.noise_info()
        assert noise["max_pbs_input_noise"] <= noise["budget"], pattern
    if params.msg_mod == 16:
        # /[0-9]x/ unanchored: 31 + 32 class lookups, 31 joins, the OR of 31 bits in one lookup
        assert _plan("matches_clear", 32, 0, b"/[0-9]x/", params=params).info()["n_pbs"] == 31 + 32 + 31 + 1


def test_whole_character_route_decrypts_like_re():
    """A toy set with 4-bit blocks (PARAM_MESSAGE_4_CARRY_4's shape): the class bit is one lookup on the whole character."""
    import fhestr
    from conftest import keyset
    p, cap = O.TOY_N32768, 4
    ks = keyset(p)
    for pattern, strings in ((b"/[b-d]+x$/", [b"", b"bx", b"bxa", b"acdx"]), (b"/^.[^a]?$/i", [b"", b"a", b"aA", b"ab", b"abc"])):
        plan = fhestr.Plan.string_op(None, "matches_clear", cap, 0, pattern, params=_params(p))
        for s in strings:
            out = ks.ck.decrypt_many(run_with_oracle(plan, ks.ck.encrypt_many(fhestr.string_to_blocks(_params(p), s, cap)), ks.sk))
            assert int(out[0]) == has_match(s, pattern), (pattern, s)


# (op, a_cap, b_cap, clear) -> (n_pbs, n_levels) of the commit before matches was added
UNCHANGED_TOY = [("find_clear", 8, 0, b"ab", (49, 5)), ("trim_start", 8, 0, None, (215, 8)),
                 ("replace_clear", 8, 0, b"bcXY", (67, 3)), ("find", 8, 4, None, (94, 6))]
UNCHANGED_P22 = [("contains_clear", 16, 0, b"abc", (99, 3)), ("starts_with_clear", 16, 0, b"abc", (7, 2)), ("ends_with_clear", 16, 0, b"abc", (125, 4)),
                 ("eq_clear", 16, 0, b"abc", (35, 3)), ("trim_start", 32, 0, None, (1223, 11)), ("find", 32, 4, None, (413, 7)),
                 ("split_clear:4", 32, 0, b" ", (5510, 23))]


@pytest.mark.parametrize("params,cases", [(O.TOY_K1, UNCHANGED_TOY), (P22, UNCHANGED_P22)], ids=["toy_k1", "p22"])
def test_existing_operations_build_the_same_plans(params, cases):
    for op, a_cap, b_cap, clear, want in cases:
        info = _plan(op, a_cap, b_cap, clear, params=params).info()
        assert (info["n_pbs"], info["n_levels"]) == want, op


def test_a_lone_accepting_bit_leaves_through_a_lookup(toy_k1):
    """a_cap = 1, or one position under `$` at the last character: a single accepting bit.  For a class of more than two
    rows of the nibble table it is a sum of class-group bits, above nominal noise; like every 0/1 result it is refreshed by
    one lookup before it is the output.  /[09az]/ has three rows (0x3.: 0 and 9, 0x6.: a, 0x7.: z): two groups of
    (row id, membership mask, join) = 6 lookups, and the refresh."""
    info = _plan("matches_clear", 1, 0, b"/[09az]/", params=P22).info()
    assert (info["n_pbs"], info["n_levels"]) == (7, 3)
    assert _plan("matches_clear", 1, 0, b"/[0-9]/", params=P22).info()["n_pbs"] == 3        # one group: already a lookup's output
    for s, want in ((b"", 0), (b"9", 1), (b"a", 1), (b"z", 1), (b"5", 0), (b"q", 0), (b"A", 0), (b"j", 0)):
        assert _matches(toy_k1, s, b"/[09az]/", cap=1) == want == has_match(s, b"/[09az]/")
    for s, want in ((b"xxz", 1), (b"xxq", 0), (b"z", 0), (b"", 0)):
        assert _matches(toy_k1, s, b"/^..[09az]$/", cap=3) == want == has_match(s, b"/^..[09az]$/")


def test_the_readme_quick_start_pattern_is_valid(toy_k1):
    """The documented example stays a pattern the parser accepts, and gives what its comment promises."""
    import ast
    import re
    import fhestr
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    hay = ast.literal_eval(re.search(r'hay, pat = enc\((b"[^"]*"), 32\)', readme).group(1))
    found = re.findall(r'ops\.matches\(hay, (b"(?:[^"\\]|\\.)*")\)', readme)
    assert len(found) == 1
    pattern = ast.literal_eval(found[0])
    assert fhestr.regex_check(pattern)["positions"] > 0
    assert has_match(hay, pattern) == 1
    assert _matches(toy_k1, hay, pattern, cap=32) == 1
    assert _matches(toy_k1, hay.replace(b"quick", b"quack"), pattern, cap=32) == 0
