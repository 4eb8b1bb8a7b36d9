"""String programs without a GPU: several FheString operations recorded into one offline plan on TOY_K1
(fhestr.StringProgram over the fhe_str_program_* entry points), stepped by the CPU oracle.  What a program must decrypt
to is composed from Python `bytes` and the clear-text definitions of tests/split_ref.py, tests/count_ref.py and
tests/regex_ref.py, never from the code under test."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from count_ref import repeat_ref
from plan_oracle import run_with_oracle
from regex_ref import has_match
from split_ref import split_ref
from test_split_cpu import COMMA_STRINGS, _run_two_ranks

A_CAP, P_CAP = 8, 4
DIGITS = b"/^[0-9]+$/"


def _params():
    return to_fhestr_params(O.TOY_K1)


def _program(dedupe=True):
    import fhestr
    return fhestr.StringProgram(None, params=_params(), dedupe=dedupe)


def _enc(ks, s, cap):
    import fhestr
    return ks.ck.encrypt_many(fhestr.string_to_blocks(_params(), s, cap))


def _enc_count(ks, n, n_max):
    import fhestr
    return ks.ck.encrypt_many(fhestr.encode_count(_params(), n, n_max))


def _run(ks, compiled, inputs, run=run_with_oracle):
    """The decrypted results of a compiled program, cut by its output layout: bit -> int, string -> bytes, count -> int,
    split -> (count, [parts])."""
    import fhestr
    msgs = ks.ck.decrypt_many(run(compiled.plan, np.concatenate(inputs), ks.sk)).reshape(-1, 1)

    def clear(x):
        if isinstance(x, fhestr.SplitResult):
            return clear(x.count), [clear(p) for p in x.parts]
        if isinstance(x, fhestr.EncryptedCount):
            return fhestr.decode_count(_params(), x.digits)
        x = np.asarray(x)
        return int(x.reshape(-1)[0]) if x.size == 1 else fhestr.blocks_to_string(_params(), x)

    return tuple(clear(x) for x in compiled.results_of(msgs))


# one name of every family: (plan name, operands -- a capacity or ("count", n_max) --, clear operand)
FAMILIES = [
    ("eq", (8, 4), None), ("contains_clear", (8,), b"ab"), ("find", (8, 4), None), ("lt", (8, 4), None), ("to_lower", (8,), None),
    ("strip", (8,), None), ("concat", (8, 4), None), ("strip_prefix", (8, 4), None), ("replace:2:8", (8, 2, 2), None),
    ("replacen_encn_clear:2:1:8", (8, ("count", 2)), b"bXY"), ("split_clear:2", (8,), b","), ("rsplit_once", (8, 4), None),
    ("repeat:2", (8, ("count", 2)), None), ("matches_clear", (8,), DIGITS), ("len", (8,), None),
]
# what FheStringOps returns for the same calls: (kind, blocks, capacity / n_max) of every result, 4 blocks per
# character, counts in as many base-4 digits as their largest value needs
LAYOUTS = {
    "eq": [("bit", 1, 1)], "contains_clear": [("bit", 1, 1)], "find": [("bit", 1, 1), ("count", 2, 8)], "lt": [("bit", 1, 1)],
    "to_lower": [("string", 32, 8)], "strip": [("string", 32, 8)], "concat": [("string", 48, 12)],
    "strip_prefix": [("bit", 1, 1), ("string", 32, 8)], "replace:2:8": [("string", 32, 8)],
    "replacen_encn_clear:2:1:8": [("string", 32, 8)], "split_clear:2": [("count", 1, 3), ("string", 32, 8), ("string", 32, 8)],
    "rsplit_once": [("bit", 1, 1), ("string", 32, 8), ("string", 32, 8)], "repeat:2": [("string", 64, 16)],
    "matches_clear": [("bit", 1, 1)], "len": [("count", 2, 8)],
}


def _one_op(name, operands, clear, dedupe):
    prog = _program(dedupe)
    values = [prog.count(o[1]) if isinstance(o, tuple) else prog.string(o) for o in operands]
    results = prog.op(name, *values, clear=clear)
    prog.output(*results)
    return prog.compile(), results


def _string_op(name, operands, clear):
    import fhestr
    caps = [o for o in operands if not isinstance(o, tuple)]
    return fhestr.Plan.string_op(None, name, caps[0], sum(caps[1:]), clear, params=_params())


@pytest.mark.parametrize("name,operands,clear", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_binding_adds_nothing(name, operands, clear):
    """A one-op program without hash-consing IS the operation's plan; with it, it is never larger."""
    ref = _string_op(name, operands, clear)
    plain, _ = _one_op(name, operands, clear, dedupe=False)
    assert plain.plan.info() == ref.info()
    assert plain.plan.noise_info()["max_pbs_input_noise"] == ref.noise_info()["max_pbs_input_noise"]
    for l in range(ref.info()["n_levels"] + 1):
        a, b = plain.plan.export_level(l), ref.export_level(l)
        assert all(np.array_equal(a[k], b[k]) for k in ("off", "src", "coeff", "cst", "lut")), (name, l)
    shared, _ = _one_op(name, operands, clear, dedupe=True)
    assert shared.plan.info()["n_pbs"] <= ref.info()["n_pbs"]
    assert shared.plan.info()["n_levels"] <= ref.info()["n_levels"]
    assert shared.plan.noise_info()["max_pbs_input_noise"] <= ref.noise_info()["budget"]


@pytest.mark.parametrize("name,operands,clear", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_layout_table(name, operands, clear):
    compiled, results = _one_op(name, operands, clear, dedupe=True)
    assert [(r.kind, r.blocks, r.extent) for r in results] == LAYOUTS[name]
    assert sum(r.blocks for r in results) == _string_op(name, operands, clear).info()["n_outputs"]
    assert all(r.op == 0 for r in results) and all(v.op is None for v in compiled.inputs)


def test_layout_capacities_follow_the_plan_name():
    prog = _program()
    a, b, n = prog.string(8), prog.string(4), prog.count(2)
    assert prog.op("split_clear:3:5", a, clear=b",")[1].cap == 5
    assert [r.extent for r in prog.op("split:5", a, b)] == [6, 8, 8, 8, 8, 8]
    assert prog.op("split:5", a, b)[0].blocks == 2                          # the value 6 in two base-4 digits
    assert prog.op("replacen_encn:2:4:32", a, b, b, n)[0].cap == 32
    assert prog.repeat(a, 3).cap == 24 and prog.concat(a, b"xyz").cap == 11
    assert prog.replace(a, b"ab", b"c", out_cap=6).cap == 6 and prog.replace(a, b"ab", b"cd").cap == 8
    found, parts = prog.split_once(a, b, part_cap=3)
    assert found.kind == "bit" and [p.cap for p in parts] == [3, 3]
    assert prog.find(a, b"x")[1].n_max == 8 and prog.len(b).n_max == 4 and prog.len(b).blocks == 2


def _mixed(s):
    """Mixed case and surrounding blanks added, within the capacity."""
    return (b" " + bytes(c - 32 if i % 2 == 0 and 97 <= c <= 122 else c for i, c in enumerate(s)) + b"  ")[:A_CAP]


CHAIN_CASES = [(_mixed(s), p) for s in COMMA_STRINGS for p in (b"b", split_ref("split", s, b",", 2)[1][1])]


def _chain(world=1, dedupe=True):
    prog = _program(dedupe)
    a, p = prog.string(A_CAP), prog.string(P_CAP)
    parts = prog.split(prog.strip(prog.to_lower(a)), b",", 2)
    prog.output(parts, prog.eq(parts.parts[1], p))
    return prog.compile(world)


def _chain_ref(a, p):
    count, parts = split_ref("split", a.lower().strip(), b",", 2)
    return (count, parts), int(parts[1] == p)


def test_chain_decrypts_to_the_composed_python_result(toy_k1):
    """split_clear:2 of strip(to_lower(a)) on b",", then eq of part 1 with an encrypted p."""
    compiled = _chain()
    assert any(a != a.lower() for a, _ in CHAIN_CASES) and any(a != a.strip() for a, _ in CHAIN_CASES)
    for a, p in CHAIN_CASES:
        assert _run(toy_k1, compiled, [_enc(toy_k1, a, A_CAP), _enc(toy_k1, p, P_CAP)]) == _chain_ref(a, p), (a, p)
    noise = compiled.plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]


def test_chain_world_2(toy_k1):
    compiled = _chain(world=2)
    assert compiled.plan.info()["world"] == 2
    for a, p in CHAIN_CASES[2:8]:
        got = _run(toy_k1, compiled, [_enc(toy_k1, a, A_CAP), _enc(toy_k1, p, P_CAP)], run=_run_two_ranks)
        assert got == _chain_ref(a, p), (a, p)
    jobs = [sum(compiled.plan.level_rank_info(l, r)["job_hi"] - compiled.plan.level_rank_info(l, r)["job_lo"]
                for l in range(compiled.plan.info()["n_levels"])) for r in range(2)]
    assert min(jobs) > 0


ORDER = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b}


def _four(dedupe):
    prog = _program(dedupe)
    a, b = prog.string(A_CAP), prog.string(P_CAP)
    prog.output(*(getattr(prog, op)(a, b) for op in ORDER))
    return prog.compile()


def test_four_comparisons_side_by_side(toy_k1):
    """compare_sign is built once; order_bit is one lookup per comparison."""
    lt = _string_op("lt", (A_CAP, P_CAP), None).info()
    shared, plain = _four(True), _four(False)
    assert shared.plan.info()["n_pbs"] == lt["n_pbs"] + 3
    assert shared.plan.info()["n_levels"] == lt["n_levels"]
    assert plain.plan.info()["n_pbs"] == sum(_string_op(op, (A_CAP, P_CAP), None).info()["n_pbs"] for op in ORDER)
    assert plain.plan.info()["n_levels"] == lt["n_levels"]
    for a, b in ((b"abc", b"abd"), (b"abd", b"abd"), (b"abe", b"abd"), (b"ab", b"abd"), (b"abcde", b"abcd"), (b"", b""), (b"", b"a")):
        for compiled in (shared, plain):
            got = _run(toy_k1, compiled, [_enc(toy_k1, a, A_CAP), _enc(toy_k1, b, P_CAP)])
            assert got == tuple(int(f(a, b)) for f in ORDER.values()), (a, b)


def test_unrelated_operations_share_levels(toy_k1):
    prog = _program()
    a, b = prog.string(A_CAP), prog.string(A_CAP)
    prog.output(prog.matches(a, DIGITS), prog.split(b, b",", 2))
    compiled = prog.compile()
    m, s = _string_op("matches_clear", (A_CAP,), DIGITS).info(), _string_op("split_clear:2", (A_CAP,), b",").info()
    info = compiled.plan.info()
    assert info["n_levels"] == max(m["n_levels"], s["n_levels"])
    assert info["n_pbs"] == m["n_pbs"] + s["n_pbs"]
    for a_s, b_s in ((b"0123", b"a,b"), (b"12a4", b",,"), (b"", b"abc"), (b"7", b"a,b,c,d")):
        got = _run(toy_k1, compiled, [_enc(toy_k1, a_s, A_CAP), _enc(toy_k1, b_s, A_CAP)])
        assert got == (has_match(a_s, DIGITS), split_ref("split", b_s, b",", 2)), (a_s, b_s)


def test_a_hidden_count_flows_into_repeat(toy_k1):
    """repeat:4(b, len(a)), a_cap = 4: the digits of len are PBS outputs in [0, msg_mod), bound as they are."""
    def build(dedupe):
        prog = _program(dedupe)
        a, b = prog.string(4), prog.string(4)
        n = prog.len(a)
        assert (n.kind, n.n_max, n.blocks) == ("count", 4, 2)
        prog.output(prog.repeat(b, n))
        return prog.compile()

    plain, shared = build(False), build(True)
    both = _string_op("len", (4,), None).info()["n_pbs"] + _string_op("repeat:4", (4, ("count", 4)), None).info()["n_pbs"]
    assert plain.plan.info()["n_pbs"] == both          # no cleaning lookup between the two
    assert shared.plan.info()["n_pbs"] <= both
    for a, b in ((b"", b"xy"), (b"a", b"xy"), (b"abc", b"x"), (b"abcd", b"wxyz"), (b"ab", b"")):
        for compiled in (plain, shared):
            assert _run(toy_k1, compiled, [_enc(toy_k1, a, 4), _enc(toy_k1, b, 4)]) == (repeat_ref(b, len(a), 4),), (a, b)


def test_a_short_count_is_extended_and_a_long_one_refused(toy_k1):
    import fhestr
    prog = _program()
    a, n1, n20 = prog.string(4), prog.count(3), prog.count(20)
    assert (n1.blocks, n20.blocks) == (1, 3)
    prog.output(prog.op("repeat:4", a, n1)[0])          # repeat:4 takes two digits: one trivial zero digit is added
    with pytest.raises(fhestr.FheError, match="3 digits, the op takes 2"):
        prog.op("repeat:4", a, n20)
    compiled = prog.compile()
    for n in (0, 1, 3):
        got = _run(toy_k1, compiled, [_enc(toy_k1, b"ab", 4), _enc_count(toy_k1, n, 3), _enc_count(toy_k1, 0, 20)])
        assert got == (b"ab" * n,)


def test_the_cleaning_rule(toy_k1):
    """Blocks of a concat result are linear combinations of two gated blocks: more than nominal noise, no node of their
    own.  Bound to to_upper, each of them passes through one lookup first and the plan stays within the budget."""
    concat = _string_op("concat", (4, 4), None)
    out = concat.export_level(concat.info()["n_levels"])
    n_lin = sum(1 for j in range(out["jobs"]) if out["off"][j + 1] - out["off"][j] != 1 or out["coeff"][out["off"][j]] != 1)
    assert 0 < n_lin <= out["jobs"]
    prog = _program(dedupe=False)
    a, b = prog.string(4), prog.string(4)
    prog.output(prog.to_upper(prog.concat(a, b)))
    compiled = prog.compile()
    assert compiled.plan.info()["n_pbs"] == concat.info()["n_pbs"] + _string_op("to_upper", (8,), None).info()["n_pbs"] + n_lin
    noise = compiled.plan.noise_info()
    assert noise["max_pbs_input_noise"] <= noise["budget"]
    for a_s, b_s in ((b"ab", b"cd"), (b"", b"xyz"), (b"abcd", b"efgh"), (b"a-Z", b"")):
        assert _run(toy_k1, compiled, [_enc(toy_k1, a_s, 4), _enc(toy_k1, b_s, 4)]) == ((a_s + b_s).upper(),)


def test_values_of_several_kinds_flow(toy_k1):
    """find's index as the count of replacen, strip_prefix's string into contains, the same value used twice."""
    prog = _program()
    a, pat = prog.string(A_CAP), prog.string(2)
    found, index = prog.find(a, pat)
    stripped, rest = prog.strip_prefix(a, b"ab")
    prog.output(found, index, prog.replacen(a, b"a", b"XY", index, out_cap=A_CAP), stripped, prog.contains(rest, pat), prog.is_empty(rest))
    compiled = prog.compile()
    for a_s, p_s in ((b"abcabc", b"ca"), (b"abab", b"ab"), (b"xaaaa", b"zz"), (b"ab", b"b")):
        at = a_s.find(p_s)
        rest_s = a_s[2:] if a_s.startswith(b"ab") else a_s
        want = (int(at >= 0), max(at, 0), a_s.replace(b"a", b"XY", max(at, 0))[:A_CAP] if at > 0 else a_s,
                int(a_s.startswith(b"ab")), int(p_s in rest_s), int(rest_s == b""))
        assert _run(toy_k1, compiled, [_enc(toy_k1, a_s, A_CAP), _enc(toy_k1, p_s, 2)]) == want, (a_s, p_s)


# ---- refusals, by message ----
def _refused(reason, call, *args, **kw):
    import fhestr
    with pytest.raises(fhestr.FheError) as err:
        call(*args, **kw)
    assert reason in str(err.value), str(err.value)
    assert reason in fhestr.lib().fhe_last_error().decode()


def test_refused_value_ids():
    import fhestr
    one, other = _program(), _program()
    a, b = one.string(4), other.string(4)
    _refused("belongs to another program", one.op, "eq", a, b)
    _refused("belongs to another program", one.output, b)
    ghost = fhestr.ProgramValue(one, a.id)
    ghost.id = a.id + 7
    _refused("out of range", one.op, "to_lower", ghost)
    info = (C.c_uint32 * 4)()
    assert fhestr.lib().fhe_str_program_value_info(one._h, a.id + 7, info) != 0
    assert "out of range" in fhestr.lib().fhe_last_error().decode()
    assert one.to_lower(a).cap == 4                                  # the program is still usable


def test_refused_operands():
    prog = _program()
    a, b, n = prog.string(4), prog.string(4), prog.count(2)
    bit = prog.eq(a, b)
    _refused("takes 2 encrypted string operand(s), got 1", prog.op, "eq", a)
    _refused("takes 1 encrypted string operand(s), got 2", prog.op, "to_lower", a, b)
    _refused("takes 1 encrypted string operand(s), got 2", prog.op, "eq_clear", a, b, clear=b"x")
    _refused("takes 2 to 3 encrypted string operand(s), got 1", prog.op, "replace:4:8", a)
    _refused("is a bit", prog.op, "eq", a, bit)
    _refused("the first operand must be a string", prog.op, "len", n)
    _refused("takes no encrypted count", prog.op, "eq", a, b, n)
    _refused("takes an encrypted count as its last operand", prog.op, "repeat:2", a)
    _refused("an op takes its strings, then at most one count", prog.op, "repeat:2", n, a)
    _refused("the name says a `from` of 2 characters", prog.op, "replace:2:8", a, b, b)
    import fhestr
    with pytest.raises(fhestr.FheError, match="operands are values of a StringProgram"):       # (refused before the C call)
        prog.op("eq", a, b"abcd")
    assert prog.ne(a, b).kind == "bit"


def test_refused_results_cap_still_reports_the_number():
    import fhestr
    prog = _program()
    a = prog.string(8)
    ids = (C.c_uint32 * 1)(a.id)
    res, n = (C.c_uint32 * 8)(), C.c_uint32()
    clear = (C.c_uint8 * 1)(*b",")
    assert fhestr.lib().fhe_str_program_op(prog._h, b"split_clear:3", ids, 1, clear, 1, res, 2, C.byref(n)) != 0
    assert n.value == 4 and "results_cap 2 is too small, the op returns 4 values" in fhestr.lib().fhe_last_error().decode()
    assert fhestr.lib().fhe_str_program_op(prog._h, b"split_clear:3", ids, 1, clear, 1, res, 8, C.byref(n)) == 0 and n.value == 4
    prog.output(fhestr.ProgramValue(prog, res[0]))
    assert prog.compile().plan.info()["n_pbs"] == _string_op("split_clear:3", (8,), b",").info()["n_pbs"]      # built once


def test_refused_after_finish_and_without_outputs():
    prog = _program()
    a = prog.string(4)
    low = prog.to_lower(a)
    _refused("finish without outputs", prog.compile)
    prog.output(low)
    compiled = prog.compile()
    assert compiled.plan.info()["n_outputs"] == 16
    _refused("already finished", prog.op, "to_upper", a)
    _refused("already finished", prog.string, 4)
    _refused("already finished", prog.output, low)
    _refused("already finished", prog.compile)
    assert low.cap == 4 and type(low)(prog, low.id).op == 0          # value_info outlives finish


BUILDER_REFUSALS = [   # (op, operands, clear, what build_string_op says)
    ("split_clear:2", (8,), b"", "must not be empty"),
    ("split:0", (8, 4), None, "max_parts must be at least 1"),
    ("split_clear:2:0", (8,), b",", "part capacity must be > 0"),
    ("split_clear", (8,), b",", "max_parts"),
    ("replacen_clear:1:8", (8,), b"ax", "three parameters"),
    ("matches_clear", (8,), b"/a**/", "malformed pattern at byte 3"),
    ("matches", (8, 4), None, "matches takes a clear pattern"),
    ("repeat", (8, 4), None, "repeat_clear takes one clear byte"),
    ("repeat:300", (8, ("count", 300)), None, "n_max must be in 1..255"),
    ("frobnicate", (8, 4), None, "unknown string op: frobnicate"),
    ("split_clear:x", (8,), b",", "bad numeric parameter in string op"),
]


@pytest.mark.parametrize("op,operands,clear,reason", BUILDER_REFUSALS, ids=[r[0] for r in BUILDER_REFUSALS])
def test_refusals_of_the_builder_pass_through(op, operands, clear, reason):
    """The message is the one Plan.string_op gives for the same name."""
    import fhestr
    caps = [o for o in operands if not isinstance(o, tuple)]
    with pytest.raises(fhestr.FheError) as direct:
        fhestr.Plan.string_op(None, op, caps[0], sum(caps[1:]), clear, params=_params())
    prog = _program()
    values = [prog.count(o[1]) if isinstance(o, tuple) else prog.string(o) for o in operands]
    _refused(reason, prog.op, op, *values, clear=clear)
    assert str(direct.value) == fhestr.lib().fhe_last_error().decode()
    _refused("unusable since an op was refused while it was being built", prog.op, "to_lower", values[0])


def test_a_dropped_program_is_freed_at_once():
    """Values hold no reference back to their program: no cycle keeps it (and what it points into) alive until a
    collection."""
    import gc
    import weakref
    gc.disable()
    try:
        prog = _program()
        low = prog.to_lower(prog.string(4))
        prog.output(low)
        compiled = prog.compile()
        alive = weakref.ref(prog)
        del prog
        assert alive() is None
        assert low.cap == 4 and compiled.plan.info()["n_outputs"] == 16
    finally:
        gc.enable()
