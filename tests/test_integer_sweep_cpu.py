"""Every integer plan (fhe_int_plan_create) against Python integers, on the noise-free executor (tests/clear_plan.py): all 19
names, block counts 1, 2, 3, 4, 5, 8, 9, 64 / bits (+ 1 without a scalar), block widths of 1, 2, 3 and 4 bits, boxes from 4
to 256, scalars inside and beyond the integer's range.  Nothing here needs a device or a key: a plan built offline from
`params=` is run on clear messages.

Every case asserts: the decoded blocks equal the Python result block for block (so no output of add / sub / cmux keeps a
carry), no lookup input is off the centre of its box, and the plan's largest lookup-input noise is within its budget.
Every (set, boolean name) ends by asserting that both answers were met at every block count -- except for scalars beyond
the range, whose answer is fixed by construction and is compared with Python's on the unreduced scalar.

REFUSED lists every (set, name) the library refuses, from which block count on, with the phrase of its message: a refusal
outside it fails, and so does an entry that builds.  All of them have their reason in the size of the box; none in noise."""
import os
import sys
import time

import numpy as np
import pytest

import integer_cases as ic
import oracle as O
from clear_plan import ClearBackend, decode, run_clear
from conftest import ROOT, to_fhestr_params
from exact_plan import run_ranks

sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _reference_set(name):
    from noise_budget import reference_params
    return reference_params(name)


# label -> (fhestr.Params builder, share table bodies between backends).  TOY_K1: M = 4, T = 16; TOY_N32768: M = 16.
SETS = {
    "TOY_K1": (lambda: to_fhestr_params(O.TOY_K1), False),
    "TOY_N32768": (lambda: to_fhestr_params(O.TOY_N32768), True),
    "P11": (lambda: _reference_set("PARAM_MESSAGE_1_CARRY_1_KS_PBS"), False),                      # M = 2, T = 4
    "P12": (lambda: _reference_set("PARAM_MESSAGE_1_CARRY_2_KS_PBS"), False),                      # M = 2, T = 8
    "P13": (lambda: _reference_set("PARAM_MESSAGE_1_CARRY_3_KS_PBS"), False),                      # M = 2, T = 16
    "P23": (lambda: _reference_set("PARAM_MESSAGE_2_CARRY_3_KS_PBS"), True),                       # M = 4, T = 32
    "P33": (lambda: _reference_set("PARAM_MESSAGE_3_CARRY_3_KS_PBS"), True),                       # M = 8
    "P44": (lambda: _reference_set("PARAM_MESSAGE_4_CARRY_4_KS_PBS"), True),                       # M = 16
    "MB22_G2": (lambda: _reference_set("PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS"), False),
    "MB22_G3": (lambda: _reference_set("PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS"), False),
}
_PARAMS, _SHARE = {}, {}

SCAN = "packs two scan states in base 4, up to 10, beyond the box"      # 1-bit blocks: three scan states need base 4
DEGREE = "input degree 10 overflows"                                    # two comparator signs 4 * msb + lsb
# (set, name) -> (refused from this block count on, phrase)
REFUSED = {}
for _set in ("P11", "P12"):
    for _name in ("add", "sub", "scalar_add", "scalar_sub"):
        REFUSED[_set, _name] = (3, SCAN)
    for _name in ("gt", "ge", "lt", "le"):
        REFUSED[_set, _name] = (2 if _set == "P11" else 3, DEGREE)       # (P11 compares block by block: a sign per block)
        REFUSED[_set, "scalar_" + _name] = (3, DEGREE)

RANDOM = 40                                                             # cases per (set, name, block count), at least
TALLY = {"cases": 0, "plans": 0, "seconds": 0.0}


def params_of(label):
    if label not in _PARAMS:
        _PARAMS[label] = SETS[label][0]()
    return _PARAMS[label]


class Built:
    """One plan with its noise-free backend; run(msgs) -> output block messages, with the per-case assertions."""

    def __init__(self, label, name, n, scalar=0, world=1):
        import fhestr
        self.P = params_of(label)
        self.plan = fhestr.Plan.integer_op(None, name, n, scalar, world, params=self.P)
        self.backend = ClearBackend(self.plan, self.P, share=_SHARE if SETS[label][1] else None)
        noise = self.plan.noise_info()
        assert 0 < noise["budget"] and noise["max_pbs_input_noise"] <= noise["budget"], (label, name, n, scalar, noise)
        assert self.plan.info()["n_pbs"] > 0
        TALLY["plans"] += 1

    def run(self, msgs):
        out = run_clear(self.backend, [int(m) for m in msgs])
        assert self.backend.off_centre == 0
        TALLY["cases"] += 1
        return out

    def close(self):
        self.plan.close()


def build(label, name, n, scalar=0, world=1):
    """The plan, or None where REFUSED says so (the message checked); anything else is a failure."""
    import fhestr
    entry = REFUSED.get((label, name))
    if entry and n >= entry[0]:
        with pytest.raises(fhestr.FheError, match=entry[1]):
            fhestr.Plan.integer_op(None, name, n, scalar, world, params=params_of(label))
        return None
    return Built(label, name, n, scalar, world)


def check(built, name, n, bits, msgs, scalar=0):
    want = ic.reference(name, n, bits, msgs, scalar)
    got = built.run(msgs)
    assert got == want, (name, n, scalar, msgs, got, want)
    return want


def test_the_refusal_table_names_known_sets_and_names():
    assert all(s in SETS and n in ic.NAMES for s, n in REFUSED)
    assert not any("noise" in phrase for _, phrase in REFUSED.values())


@pytest.mark.parametrize("name", ic.NAMES)
@pytest.mark.parametrize("label", list(SETS))
def test_sweep(label, name):
    t0 = time.perf_counter()
    P = params_of(label)
    M, T = P.msg_mod, P.msg_mod * P.carry_mod
    bits = M.bit_length() - 1
    rng = np.random.default_rng([sorted(SETS).index(label), ic.NAMES.index(name)])
    entry = REFUSED.get((label, name))
    built_any = False
    for n in ic.block_counts(name, bits):
        answers, fixed = set(), 0
        if name in ic.SCALAR:
            for scalar, operands in ic.scalar_cases(n, bits, rng, per_scalar=7):
                b = build(label, name, n, scalar)
                if b is None:
                    break
                for a in operands:
                    want = check(b, name, n, bits, ic.to_blocks(a, n, bits), scalar)
                    if name in ic.BOOLEAN and ic.in_range(scalar, n, bits):
                        answers.add(want[0])
                    elif name in ic.BOOLEAN:
                        # decided at build: Python's comparison with the unreduced scalar, the same for every a
                        assert want == [int(name in ("scalar_ne", "scalar_lt", "scalar_le"))]
                        fixed += 1
                b.close()
            else:
                assert not (name in ic.BOOLEAN and n * bits < 64) or fixed >= 20, (label, name, n, fixed)
                if name in ("scalar_sub",):
                    for scalar in (0, (1 << (n * bits)) & ((1 << 64) - 1)):              # scalar_sub of 0 and of 2^bits
                        b = build(label, name, n, scalar)
                        for a, _ in ic.operand_pairs(n, bits, rng, 16)[:6]:
                            check(b, name, n, bits, ic.to_blocks(a, n, bits), scalar)
                        b.close()
        else:
            b = build(label, name, n)
            if b is not None:
                if name in ic.EXTRACT:
                    rows = ic.extract_inputs(n, T, M, rng, RANDOM)
                elif name == "cmux":
                    rows = ic.cmux_inputs(n, bits, rng, RANDOM)
                else:
                    rows = [ic.to_blocks(a, n, bits) + ic.to_blocks(c, n, bits) for a, c in ic.operand_pairs(n, bits, rng, RANDOM)]
                assert len(rows) >= RANDOM or name in ic.EXTRACT
                for msgs in rows:
                    want = check(b, name, n, bits, msgs)
                    if name in ic.BOOLEAN:
                        answers.add(want[0])
                if name == "cmux":
                    assert {row[0] for row in rows} == {0, 1}
                b.close()
        if b is None:
            assert entry and n >= entry[0]
            continue
        built_any = True
        assert not entry or n < entry[0], f"{label} {name} builds at {n} blocks: REFUSED says it is refused from {entry[0]} on"
        if name in ic.BOOLEAN:
            assert answers == {0, 1}, (label, name, n, answers)
    assert built_any or entry
    TALLY["seconds"] += time.perf_counter() - t0


EXHAUSTIVE = [("TOY_K1", name, 2) for name in ic.TWO_OPERAND] + [("TOY_K1", name, 3) for name in ("add", "sub", "gt", "eq")] + \
             [("P13", name, 4) for name in ("add", "sub")]


@pytest.mark.parametrize("label,name,n", EXHAUSTIVE, ids=[f"{s}-{m}-{n}" for s, m, n in EXHAUSTIVE])
def test_every_pair(label, name, n):
    """All pairs of n-block integers: 256 at two 2-bit blocks and at four 1-bit blocks, 4,096 at three 2-bit blocks."""
    t0 = time.perf_counter()
    bits = params_of(label).msg_mod.bit_length() - 1
    b = build(label, name, n)
    size = 1 << (n * bits)
    blocks = [ic.to_blocks(v, n, bits) for v in range(size)]
    answers = set()
    for a in range(size):
        for c in range(size):
            answers.add(tuple(check(b, name, n, bits, blocks[a] + blocks[c])))
    assert len(answers) == (size if name in ic.ARITH else 2)
    b.close()
    TALLY["seconds"] += time.perf_counter() - t0


@pytest.mark.parametrize("name", ic.NAMES)
def test_two_ranks_give_the_same_outputs(name):
    """Each name at 5 blocks on TOY_K1, finalised for two ranks and stepped over both (exact_plan.run_ranks): every rank
    ends with the outputs of the one-rank plan, which are Python's."""
    n, bits, scalar = 5, 2, 0x2B7 if name in ic.SCALAR else 0
    P = params_of("TOY_K1")
    rng = np.random.default_rng(ic.NAMES.index(name))
    one, two = build("TOY_K1", name, n, scalar), build("TOY_K1", name, n, scalar, world=2)
    assert two.plan.info()["world"] == 2
    rows = ic.planted_rows(name, n, bits, 16, rng, 12, scalar).tolist()
    for msgs in rows:
        want = check(one, name, n, bits, msgs, scalar)
        two.backend.reset()
        outs, _ = run_ranks(two.plan, msgs, two.backend)
        assert two.backend.off_centre == 0
        for r in range(2):
            assert decode(P, outs[r]) == want, (name, r, msgs)
        assert np.array_equal(outs[0], outs[1])
    one.close(), two.close()


def test_scalars_beyond_the_range_keep_the_inputs_and_spend_one_lookup():
    """The plan of a scalar comparison whose answer is known at build still takes the integer's blocks."""
    b = build("TOY_K1", "scalar_lt", 4, 256)
    assert (b.plan.info()["n_inputs"], b.plan.info()["n_outputs"], b.plan.info()["n_pbs"]) == (4, 1, 1)
    for name, scalar, a, want in (("scalar_lt", 256, 255, 1), ("scalar_ge", 256, 0, 0), ("scalar_eq", 256, 0, 0), ("scalar_eq", 300, 44, 0),
                                  ("scalar_ne", 300, 44, 1), ("scalar_gt", (1 << 64) - 1, 255, 0), ("scalar_le", 1 << 8, 255, 1)):
        c = build("TOY_K1", name, 4, scalar)
        assert c.run(ic.to_blocks(a, 4, 2)) == [want] == [int(ic.reference(name, 4, 2, ic.to_blocks(a, 4, 2), scalar)[0])]
        c.close()
    b.close()


def test_zz_tally():
    """Printed with -s: what the sweep above ran."""
    print(f"integer sweep: {TALLY['cases']} cases on {TALLY['plans']} plans, {TALLY['seconds']:.1f} s")
