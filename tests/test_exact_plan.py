"""The exact plan executor (tests/exact_plan.py) pinned on the CPU: on real oracle keys every pool slot and every output
word of a plan must equal the same plan stepped through the oracle's exact-integer KS + PBS, for one rank and for all
ranks of worlds 2 and 4; its numpy gather must equal the gather written on Python integers; and references made wrong on
purpose (a constant off by delta / 2, two table ids swapped) must differ, i.e. the inputs used can see such errors."""
import numpy as np
import pytest

import oracle as O
from conftest import keyset, to_fhestr_params
from exact_keyswitch import edge_big_cts
from exact_pbs import limb_terms
from exact_plan import ExactBackend, build_chain_plan, build_mixed_plan, gather_int, gather_np, run_exact, run_ranks
from plan_oracle import OracleBackend

SHAPES = [O.TOY_K1, O.TOY_K2]


def _build(name, p, world=1):
    import fhestr
    P = to_fhestr_params(p)
    string = lambda op, a, b=0, clear=None: fhestr.Plan.string_op(None, op, a, b, clear, world, params=P)
    integer = lambda op, blocks, scalar=0: fhestr.Plan.integer_op(None, op, blocks, scalar, world, params=P)
    if name in ("mixed", "mixed_hinted"):
        return build_mixed_plan(fhestr.Plan(None, params=P), world, hints=name == "mixed_hinted")
    if name == "chain":
        return build_chain_plan(fhestr.Plan(None, params=P), max(world, 2))
    return {"eq": lambda: string("eq", 3, 3), "contains": lambda: string("contains", 3, 2), "find": lambda: string("find", 3, 2),
            "to_lower": lambda: string("to_lower", 2), "replace_clear": lambda: string("replace_clear", 3, 0, b"abxy"),
            "contains_clear": lambda: string("contains_clear", 3, 0, b"a"), "find_clear": lambda: string("find_clear", 3, 0, b"a"),
            "len": lambda: string("len", 3), "int_lt": lambda: integer("lt", 4), "int_scalar_add": lambda: integer("scalar_add", 3, p.msg_mod + 1),
            "int_cmux": lambda: integer("cmux", 2), "int_scalar_eq": lambda: integer("scalar_eq", 4, 5)}[name]()


# TOY_K2 has one-bit blocks and a message+carry space of 4: the builders refuse contains / find with an encrypted pattern,
# to_lower and the radix comparisons and additions there (input degree or noise beyond the space), so that shape takes the
# clear-pattern forms, len, and the integer operations that do build.
PLANS = {O.TOY_K1.name: ["eq", "contains", "find", "to_lower", "replace_clear", "int_lt", "int_scalar_add", "mixed", "mixed_hinted"],
         O.TOY_K2.name: ["eq", "contains_clear", "find_clear", "len", "replace_clear", "int_cmux", "int_scalar_eq", "mixed", "mixed_hinted"]}
CASES = [(p, name) for p in SHAPES for name in PLANS[p.name]]
# eq and contains reduce their comparison bits one slice of the characters per rank (csrc/str_ops.h: owner_for, then
# all_true / any_true per slice), so for world > 1 they are ANOTHER circuit than for world 1 (TOY_K1, world 2: eq 7 PBS
# against 9, contains 16 against 17) and their words differ.  Every other plan here is one circuit in every world: its
# outputs must equal world 1's word for word.
OTHER_CIRCUIT_PER_WORLD = ["eq", "contains", "contains_clear"]


def _inputs(p, plan, seed):
    """Not encryptions: the structured rows of edge_big_cts first, uniformly random full-range words after them."""
    rng = np.random.default_rng([p.N, p.k, seed])
    return edge_big_cts(p, rng, plan.info()["n_inputs"])


def _exact(plan, ks, gather=gather_np):
    return ExactBackend(plan, ks.params, ks.sk.ksk, limb_terms(ks.sk.bsk.reshape(ks.params.n, ks.params.pbs_level, ks.params.k + 1,
                                                                                 ks.params.k + 1, ks.params.N)), gather=gather)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} of {len(want)} rows differ (first {bad[:8].tolist()}), {int((got != want).sum())} words"


@pytest.mark.parametrize("world", [1, 2, 4], ids=lambda w: f"world{w}")
@pytest.mark.parametrize("p,name", CASES, ids=[f"{p.name}-{name}" for p, name in CASES])
def test_exact_executor_equals_the_oracles_exact_path(p, name, world):
    """Every rank's whole pool and outputs, exact executor against oracle exact; every rank's outputs against world 1."""
    ks = keyset(p, fourier=False)
    plan = _build(name, p, world)
    inputs = _inputs(p, plan, 1)
    outs, pools = run_ranks(plan, inputs, _exact(plan, ks))
    o_outs, o_pools = run_ranks(plan, inputs, OracleBackend(plan, ks.sk, exact=True))
    for r in range(world):
        _same(pools[r], o_pools[r], f"{name} world {world} rank {r} pool")
        _same(outs[r], o_outs[r], f"{name} world {world} rank {r} outputs")
    assert plan.info()["n_pbs"] == 0 or any(pool[plan.info()["n_inputs"]:].any() for pool in pools)
    for r in range(1, world):
        _same(outs[r], outs[0], f"{name} world {world} rank {r} outputs against rank 0")
    if world > 1 and name not in OTHER_CIRCUIT_PER_WORLD:
        single = _build(name, p, 1)
        assert (single.info()["n_pbs"], single.info()["n_levels"]) == (plan.info()["n_pbs"], plan.info()["n_levels"])
        want, _ = run_exact(single, inputs, _exact(single, ks))
        _same(outs[0], want, f"{name} world {world} outputs against world 1")


@pytest.mark.parametrize("world", [2, 4], ids=lambda w: f"world{w}")
def test_level_without_exports(world):
    """build_chain_plan: level 1 exports nothing, slots a rank neither owns nor receives stay zero, all ranks agree."""
    p = O.TOY_K1
    ks = keyset(p, fourier=False)
    plan = _build("chain", p, world)
    assert [plan.level_info(l)["e_max"] for l in range(2)] == [0, 1]
    inputs = _inputs(p, plan, 5)
    outs, pools = run_ranks(plan, inputs, _exact(plan, ks))
    o_outs, o_pools = run_ranks(plan, inputs, OracleBackend(plan, ks.sk, exact=True))
    lv = plan.level_info(0)
    for r in range(world):
        _same(pools[r], o_pools[r], f"rank {r} pool")
        _same(outs[r], outs[0], f"rank {r} outputs")
        assert pools[r][lv["local_base"]: lv["local_base"] + 2].all(axis=1).any()
    assert not np.array_equal(pools[0][lv["local_base"]], pools[1][lv["local_base"]])       # the same slot, each rank its own data


@pytest.mark.parametrize("p", SHAPES, ids=lambda p: p.name)
def test_world_1_through_the_sharded_runner(p):
    """ExactBackend under ShardedPlanRunner (the product's control flow) gives what the lockstep loop gives."""
    ks = keyset(p, fourier=False)
    plan = _build("mixed", p)
    inputs = _inputs(p, plan, 2)
    out, pool = run_exact(plan, inputs, _exact(plan, ks))
    outs, pools = run_ranks(plan, inputs, _exact(plan, ks))
    _same(out, outs[0], "outputs")
    _same(pool, pools[0], "pool")


@pytest.mark.parametrize("p,name", [(O.TOY_K1, "mixed"), (O.TOY_K1, "find"), (O.TOY_K1, "int_lt"), (O.TOY_K2, "mixed"),
                                    (O.TOY_K2, "find_clear"), (O.TOY_K2, "int_cmux")], ids=lambda v: getattr(v, "name", v))
def test_numpy_gather_equals_python_integers(p, name):
    """gather_np against gather_int on every level of a plan (output gather included), over a pool of full-range words;
    then the whole plan executed with either."""
    ks = keyset(p, fourier=False)
    plan = _build(name, p)
    info = plan.info()
    rng = np.random.default_rng([p.N, 3])
    pool = rng.integers(0, 2**64, size=(info["pool_slots"], p.big_size), dtype=np.uint64)
    pool[0], pool[-1] = 2**64 - 1, 2**63
    negative = False
    for l in range(info["n_levels"] + 1):
        lv = plan.export_level(l)
        negative |= bool((lv["coeff"] < 0).any())
        jobs = list(range(lv["jobs"]))
        _same(gather_np(pool, lv, jobs), gather_int(pool, lv, jobs), f"{name} level {l}")
    assert negative or name != "mixed"
    inputs = _inputs(p, plan, 3)
    a, pa = run_exact(plan, inputs, _exact(plan, ks, gather_np))
    b, pb = run_exact(plan, inputs, _exact(plan, ks, gather_int))
    _same(a, b, "outputs")
    _same(pa, pb, "pool")


def test_mixed_plan_holds_what_it_promises():
    """A box source under a negative coefficient (constant = cst * delta - delta / 2), two jobs of a level on one table,
    two tables with one accumulator, a trivial PBS folded into a constant output."""
    p = O.TOY_K1
    plan = _build("mixed", p)
    delta = p.delta
    luts = plan.export_luts()
    same_acc = [(i, j) for i in luts for j in luts if i < j and np.array_equal(luts[i], luts[j])]
    assert len(same_acc) == 1
    levels = [plan.export_level(l) for l in range(plan.info()["n_levels"] + 1)]
    assert plan.info()["n_levels"] == 3
    l0 = levels[0]["lut"].tolist()
    assert len(l0) == 4 and len(set(l0)) == 3                         # a and b share a table
    assert set(same_acc[0]) & set(levels[1]["lut"].tolist())          # the twin table is in use
    out = levels[-1]
    # output 3 = 1 - box: coefficient -1 on a half-delta source; output 4 = the trivial PBS (no terms)
    assert out["off"][4] - out["off"][3] == 1 and out["coeff"][out["off"][3]] == -1
    assert int(out["cst"][3]) == (delta - delta // 2) % 2**64
    assert out["off"][5] == out["off"][4] and int(out["cst"][4]) % delta == 0
    f = levels[2]
    j = next(j for j in range(f["jobs"]) if (f["coeff"][f["off"][j]: f["off"][j + 1]] < 0).any())
    assert int(f["cst"][j]) == (delta - delta // 2) % 2**64


@pytest.mark.parametrize("p", SHAPES, ids=lambda p: p.name)
def test_wrong_references_differ(p):
    """Negative control: a reference with delta / 2 added to one job's constant, and one with two table ids of a level
    swapped, differ from the correct one on these inputs -- in the outputs, not only inside the pool."""
    ks = keyset(p, fourier=False)
    plan = _build("mixed", p)
    inputs = _inputs(p, plan, 4)
    want, pool = run_exact(plan, inputs, _exact(plan, ks))
    for level in range(plan.info()["n_levels"] + 1):
        wrong = _exact(plan, ks)
        wrong.levels[level]["cst"][0] += np.uint64(p.delta // 2)
        got, _ = run_exact(plan, inputs, wrong)
        assert not np.array_equal(got, want), f"cst + delta / 2 at level {level} goes unseen"
    for level in range(plan.info()["n_levels"]):
        wrong = _exact(plan, ks)
        lut = wrong.levels[level]["lut"]
        a, b = next((a, b) for a in range(len(lut)) for b in range(len(lut)) if lut[a] != lut[b]
                    and not np.array_equal(wrong.luts[lut[a]], wrong.luts[lut[b]]))
        lut[a], lut[b] = lut[b], lut[a]
        got, _ = run_exact(plan, inputs, wrong)
        assert not np.array_equal(got, want), f"table ids swapped at level {level} go unseen"
