"""The noise-free plan executor (tests/clear_plan.py) pinned before anything trusts it: on real TOY_K1 keys every pool slot
of deep string plans decrypts, through the CPU oracle, to the executor's phase within a quarter of a box; hand-built plans
(exact_plan.build_mixed_plan / build_chain_plan: a signed PBS, a full-box node read through a negative coefficient, a PBS of
a trivial input, twin tables with one accumulator, a level without a collective) give what their node definitions, written
out here in plain Python, give -- for all msg_mod^4 inputs, and on every rank of worlds 1, 2 and 4; its level-at-a-time
gather equals exact_plan.gather_np and gather_int; and an executor made wrong on purpose (one coefficient, one constant,
one table id of the exports edited) is noticed, by the outputs or by the rule that every PBS input is a multiple of delta."""
import itertools

import numpy as np
import pytest

import oracle as O
import plan_cases as pc
from clear_plan import ClearBackend, decode, gather_flat, run_clear
from conftest import to_fhestr_params
from exact_plan import build_chain_plan, build_mixed_plan, gather_int, gather_np, run_ranks
from plan_oracle import OracleBackend

P = O.TOY_K1
M, T = P.msg_mod, P.msg_mod * P.carry_mod
DELTA = (1 << 63) // T


def _params():
    return to_fhestr_params(P)


def _string_plan(op, a_cap, b_cap=0, clear=None, world=1):
    import fhestr
    return fhestr.Plan.string_op(None, op, a_cap, b_cap, clear, world, params=_params())


def _blocks(*operands):
    codec = pc.Codec(P)
    return [v for x in operands for v in (codec.blocks(*x) if isinstance(x, tuple) else x)]


# (name, build, clear input messages): the deep plans of the issue, capacity 8
DEEP = [
    ("replace:2:9", lambda: _string_plan("replace:2:9", 8, 4), _blocks((b"abcabc", 8), (b"bc", 2), (b"XY", 2))),
    ("rsplit:3", lambda: _string_plan("rsplit:3", 8, 2), _blocks((b"a,b,,c", 8), (b",", 2))),
    ("matches_clear", lambda: _string_plan("matches_clear", 8, 0, b"/a(b|c)+d$/"), _blocks((b"xabcbd", 8))),
    ("rsplitn_encn:3", lambda: _string_plan("rsplitn_encn:3", 8, 2), _blocks((b"a,b,,c", 8), (b",", 2), [2])),
    ("program of three", lambda: pc.three_step_program(_params()).plan, _blocks((b" A,Cd,e ", 8))),
]


@pytest.mark.parametrize("name,build,msgs", DEEP, ids=[d[0] for d in DEEP])
def test_every_pool_slot_agrees_with_the_oracle(toy_k1, name, build, msgs):
    """Real encryptions through OracleBackend, clear messages through ClearBackend: for EVERY pool slot the signed torus
    distance between the oracle's decrypted phase and the clear phase is below delta / 4 -- the bound is the decision
    margin (half of the half box), not a fitted number; the noise of TOY_K1 measured at most 0.0014 of delta / 2."""
    plan = build()
    info = plan.info()
    assert len(msgs) == info["n_inputs"]
    _, (o_pool,) = run_ranks(plan, toy_k1.ck.encrypt_many(msgs), OracleBackend(plan, toy_k1.sk))
    backend = ClearBackend(plan, _params())
    outs, (pool,) = run_ranks(plan, msgs, backend)
    phase = np.array([toy_k1.ck.decrypt_plaintext(o_pool[s]) for s in range(info["pool_slots"])], dtype=np.uint64)
    err = (phase - pool[:, 0]).astype(np.int64)
    worst = int(np.abs(err).argmax())
    print(f"{name}: {info['pool_slots']} slots, {info['n_levels']} levels, worst |error| {abs(int(err[worst])) / (DELTA / 2):.5f} of delta / 2 at slot {worst}")
    assert np.abs(err).max() < DELTA // 4, (name, worst)
    assert backend.n_pbs == info["n_pbs"] and backend.off_centre == 0
    assert pool[info["n_inputs"]:].any()
    decode(_params(), outs[0])


def test_deep_plans_decode_to_their_references():
    """What the five plans above compute, for the inputs above (so the slots compared there are slots of right answers)."""
    codec = pc.Codec(P)
    out = {name: run_clear(ClearBackend(build(), _params()), msgs) for name, build, msgs in DEEP}
    assert codec.text(out["replace:2:9"]) == b"abcabc".replace(b"bc", b"XY")
    assert pc.decode_split("rsplit", out["rsplit:3"], M, 3, 8) == pc.split_ref("rsplit", b"a,b,,c", b",", 3)
    assert out["matches_clear"] == [pc.has_match(b"xabcbd", b"/a(b|c)+d$/")] == [1]
    assert pc.decode_split("splitn", out["rsplitn_encn:3"], M, 3, 8) == pc.splitn_ref("rsplitn", b"a,b,,c", b",", 2, 3)
    assert codec.text(out["program of three"]) == pc.three_step_reference(b" A,Cd,e ") == b"cd,e"


# ---- hand-built plans against their node definitions ---------------------------------------------------------------

def mixed_reference(x):
    """exact_plan.build_mixed_plan, node by node (values modulo 2T as the outputs decode)."""
    flip = lambda v: (T - 1 - v) % M
    a, b, c = (x[0] + x[1]) % M, x[2] % M, flip(x[3])
    d = (x[0] > x[1]) - (x[0] < x[1])                  # the signed PBS: an odd table read through its negacyclic extension
    box = int(a + b != 0)                              # the full box, stored as box - 1/2
    e = (c + d + 1) % M                                # `twin`: values 2T apart from `ident`, the same accumulator
    t = flip(2)                                        # the PBS of a trivial input, folded at build time
    f = flip(c + 1 - box)                              # the box through a negative coefficient
    g = (box + t) % M
    return [f, g, e, 1 - box, t]


def chain_reference(x, world):
    up, flip = lambda v: (v + 1) % M, lambda v: (T - 1 - v) % M
    ends = [(flip if r % 2 else up)(up(x[r] + x[r + 1]) + flip(x[r])) for r in range(world)]
    return ends + [((M - 1) * ends[0] - ends[-1] + M - 1) % (2 * T)]


@pytest.mark.parametrize("hints", [False, True], ids=["auto", "hinted"])
@pytest.mark.parametrize("world", [1, 2, 4], ids=lambda w: f"world{w}")
def test_mixed_plan_all_inputs_against_the_node_definitions(world, hints):
    """All msg_mod^4 = 256 input combinations, every rank."""
    import fhestr
    plan = build_mixed_plan(fhestr.Plan(None, params=_params()), world, hints=hints)
    backend = ClearBackend(plan, _params())
    padding = 0
    for x in itertools.product(range(M), repeat=4):
        backend.reset()
        outs, _ = run_ranks(plan, list(x), backend)
        for r in range(world):
            assert decode(_params(), outs[r]) == mixed_reference(x), (x, world, r)
        assert backend.off_centre == 0
        padding += backend.padding
    assert padding > 0                                  # x0 < x1 puts the signed PBS's input on the padding bit


@pytest.mark.parametrize("world", [2, 4], ids=lambda w: f"world{w}")
def test_chain_plan_without_a_collective(world):
    import fhestr
    plan = build_chain_plan(fhestr.Plan(None, params=_params()), world)
    assert plan.level_info(0)["e_max"] == 0 and plan.level_info(1)["e_max"] > 0
    backend = ClearBackend(plan, _params())
    rng = np.random.default_rng(5)
    for x in [[0] * (world + 1), [M - 1] * (world + 1)] + rng.integers(0, M, size=(30, world + 1)).tolist():
        backend.reset()
        outs, _ = run_ranks(plan, x, backend)
        for r in range(world):
            assert decode(_params(), outs[r]) == chain_reference(x, world), (x, world, r)
        assert backend.off_centre == 0 and backend.n_pbs == plan.info()["n_pbs"]


@pytest.mark.parametrize("name", ["mixed", "find", "replace_clear"])
@pytest.mark.parametrize("world", [2, 4], ids=lambda w: f"world{w}")
def test_every_rank_equals_world_1(world, name):
    """The same circuit in every world: every rank's outputs are world 1's, word for word."""
    import fhestr
    build = {"mixed": lambda w: build_mixed_plan(fhestr.Plan(None, params=_params()), w, hints=True),
             "find": lambda w: _string_plan("find", 3, 2, None, w),
             "replace_clear": lambda w: _string_plan("replace_clear", 4, 0, b"abxy", w)}[name]
    rng = np.random.default_rng(9)
    single, plan = build(1), build(world)
    for _ in range(8):
        msgs = rng.integers(0, M, size=plan.info()["n_inputs"]).tolist()
        (want,), _ = run_ranks(single, msgs, ClearBackend(single, _params()))
        outs, _ = run_ranks(plan, msgs, ClearBackend(plan, _params()))
        for r in range(world):
            assert np.array_equal(outs[r], want), (name, world, r, msgs)


def test_gathers_agree_on_width_1_pools():
    """gather_flat (a level at a time) against gather_np and gather_int, on full-range words: every level of a deep plan
    and of the mixed plan (negative coefficients, constants with a half-delta share)."""
    import fhestr
    rng = np.random.default_rng(3)
    for plan in (_string_plan("replace:2:9", 8, 4), build_mixed_plan(fhestr.Plan(None, params=_params()))):
        info = plan.info()
        pool = rng.integers(0, 2**64, size=(info["pool_slots"], 1), dtype=np.uint64)
        negative = 0
        for l in range(info["n_levels"] + 1):
            lv = plan.export_level(l)
            jobs = list(range(lv["jobs"]))
            want = gather_int(pool, lv, jobs)
            assert np.array_equal(gather_np(pool, lv, jobs), want) and np.array_equal(gather_flat(pool, lv, jobs), want), l
            part = jobs[1::2]
            assert np.array_equal(gather_flat(pool, lv, part), want[1::2])
            negative += int((lv["coeff"] < 0).sum())
        assert negative > 0


# ---- the executor can fail ------------------------------------------------------------------------------------------

def _detected(plan, msgs, want, edit):
    """An executor whose exports `edit` changed: True iff its outputs differ, a PBS input leaves the multiples of delta, or
    an output does."""
    backend = ClearBackend(plan, _params())
    edit(backend)
    outs, _ = run_ranks(plan, msgs, backend)
    try:
        return decode(_params(), outs[0]) != want or backend.off_centre > 0
    except AssertionError:
        return True


def test_an_edited_export_is_noticed():
    """Every lookup of find (capacity 8, pattern capacity 2) in turn gets (a) its first coefficient raised by one, (b) its
    constant moved by delta / 2 -- a Node::half share folded into the wrong place --, (c) its constant moved by delta,
    (d) another table.  (b) must be noticed at EVERY lookup, by the multiple-of-delta rule alone; of the others, which an
    input may mask (a term whose source is 0, a lookup whose result the answer does not depend on for this string), at
    least one lookup each -- and the unedited executor is not "noticed"."""
    plan = _string_plan("find", 8, 2)
    msgs = _blocks((b"xxabxab", 8), (b"ab", 2))
    want = run_clear(ClearBackend(plan, _params()), msgs)
    assert (want[0], pc.Codec(P).number(want[1:])) == (1, 2)
    assert not _detected(plan, msgs, want, lambda b: None)
    n_luts = len(ClearBackend(plan, _params()).bodies)
    assert n_luts > 1
    hits = {"coefficient": 0, "half": 0, "constant": 0, "table": 0}
    jobs = [(l, j) for l in range(plan.info()["n_levels"]) for j in range(plan.level_info(l)["jobs"])]
    for l, j in jobs:
        def coefficient(b):
            b.levels[l]["coeff"][b.levels[l]["off"][j]] += 1

        def half(b):
            b.levels[l]["cst"][j] += np.uint64(DELTA // 2)

        def constant(b):
            b.levels[l]["cst"][j] += np.uint64(DELTA)

        def table(b):
            b.levels[l]["lut"][j] = (b.levels[l]["lut"][j] + 1) % n_luts

        for name, edit in (("coefficient", coefficient), ("half", half), ("constant", constant), ("table", table)):
            with np.errstate(over="ignore"):
                hits[name] += _detected(plan, msgs, want, edit)
    print(f"{len(jobs)} lookups; edits noticed: {hits}")
    assert hits["half"] == len(jobs)
    assert hits["coefficient"] and hits["constant"] and hits["table"]


def test_decode_refuses_an_off_centre_phase():
    assert decode(_params(), [3 * DELTA, (2 * T - 1) * DELTA]) == [3, 2 * T - 1]
    with pytest.raises(AssertionError):
        decode(_params(), [3 * DELTA + DELTA // 2])
