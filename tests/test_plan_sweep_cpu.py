"""Every FheString plan against byte semantics, on the CPU, through the noise-free executor (tests/clear_plan.py).

The exact-integer GPU tests pin the executor against the plan; nothing there notices a plan that is wrong -- a value range
asserted too narrow (Circuit::lin's degree_override), a Node::half share folded into the wrong constant, a table built for
the wrong digit: such a plan builds, runs bit for bit as exported, and answers wrongly for the inputs that reach the
mistake.  Here each operation meets thousands of inputs (tests/plan_cases.py: exhaustive small alphabets, then random
cases over capacities 1 .. 33 with positives, overlaps and near misses made frequent), on TOY_K1 (2-bit blocks, T = 16)
and TOY_N32768 (4-bit blocks, T = 256: the whole-character circuits), and every case asserts

    the decoded outputs equal the reference (Python `bytes`, split_ref, count_ref, regex_ref -- never the library),
    no PBS input is off a multiple of delta (a padding-bit input is fine: signed lookups and full boxes have them),
    the plan built (the generators draw only what the library accepts: a refusal fails and names the plan),
    the plan's declared worst PBS-input noise is what its exported levels carry, and within the budget.

Each family ends by asserting that both answers of every boolean result and every capacity of its list were met.

Counts: the issue's, at the rates measured on this code (TOY_K1: 1,500 to 10,000 cases/s once a plan is built, 150 to 400
plan builds/s), except family 3 on TOY_N32768, 1,500 cases instead of 3,000: every plan there exports tables of 2 x 32768
words, and 3,000 cases took 53 s."""
import pytest

import oracle as O
import plan_cases as pc

SETS = {p.name: p for p in (O.TOY_K1, O.TOY_N32768)}
P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
_CODECS = {}


def _codec(name):
    if name not in _CODECS:
        _CODECS[name] = pc.Codec(SETS.get(name, P22))
    return _CODECS[name]


def _report(sweep, what):
    print(f"{sweep.codec.name} {what}: {sweep.cases} cases on {len(sweep.backends)} plans, {sweep.n_pbs} PBS inputs "
          f"({sweep.padding} with the padding bit), worst declared noise {sweep.worst_noise}")


by_set = pytest.mark.parametrize("name", list(SETS))


@by_set
@pytest.mark.parametrize("op", pc.COMPARE_OPS)
def test_family1_comparisons_and_searches(name, op):
    """40 x 40 pairs over {a, b, B} at capacity 3 (every pair encrypted, and in one other form), then 125 random cases
    (1,500 over the twelve operations) over the capacity list, in all four forms."""
    sweep = pc.Sweep(_codec(name))
    for case in pc.family1_exhaustive(sweep.codec, op):
        sweep.check(case)
    assert sweep.cases == 2 * 40 * 40
    for case in pc.family1_random(sweep.codec, op, 125):
        sweep.check(case)
    _report(sweep, op)
    sweep.assert_coverage()


@by_set
@pytest.mark.parametrize("op", pc.SHAPE_OPS)
def test_family2_unary_and_shape_changing(name, op):
    """All 341 strings of length <= 4 over {a, A, ' ', newline} at capacities 4 and 5, then 91 random cases (1,000 over the
    eleven operations)."""
    sweep = pc.Sweep(_codec(name))
    for case in pc.family2_exhaustive(sweep.codec, op):
        sweep.check(case)
    assert sweep.cases == 2 * 341
    for case in pc.family2_random(sweep.codec, op, 91):
        sweep.check(case)
    _report(sweep, op)
    sweep.assert_coverage()


@by_set
def test_family3_split_and_replace(name):
    sweep = pc.Sweep(_codec(name))
    for case in pc.family3(sweep.codec, 3000 if name == O.TOY_K1.name else 1500):
        sweep.check(case)
    _report(sweep, "split and replace")
    sweep.assert_coverage()
    assert {"split_once", "rsplit_once"} <= set(sweep.seen_bits)


@by_set
def test_family4_encrypted_counts(name):
    sweep = pc.Sweep(_codec(name))
    for case in pc.family4(sweep.codec, 600):
        sweep.check(case)
    _report(sweep, "encrypted counts")
    sweep.assert_coverage()


@by_set
def test_family5_matches_clear(name):
    sweep = pc.Sweep(_codec(name))
    for case in pc.family5(sweep.codec, 600):
        sweep.check(case)
    assert sweep.cases == 3600
    _report(sweep, "matches_clear")
    sweep.assert_coverage(pc.REGEX_CAPS)


@by_set
def test_family6_string_programs(name):
    """300 random chains, four inputs each; a case whose intermediate result a capacity cuts is left out (replace into
    capacity + 2 is the only step that can cut), at most 2 % of them."""
    sweep = pc.Sweep(_codec(name))
    cut = total = 0
    for case, is_cut in pc.family6(sweep.codec, 300):
        total += 1
        if is_cut:
            cut += 1
            sweep.backend(case)                # the plan still has to build, and to keep its noise books
        else:
            sweep.check(case)
    _report(sweep, f"programs ({cut} of {total} cases left out as cut)")
    assert total == 1200 and cut <= 0.02 * total
    sweep.assert_coverage(pc.PROGRAM_CAPS)
    assert {"program eq", "program contains", "program find"} <= set(sweep.seen_bits)
    assert {k[-1] for k in sweep.backends} == {True, False}               # dedupe on and off
    twice = sum(1 for k in sweep.backends if sum(s.endswith("_w") for s in k[4]) + (k[5] == "contains") >= 2)
    assert twice >= 30, twice                                              # the second input consumed twice


@pytest.mark.parametrize("world", [2, 4], ids=lambda w: f"world{w}")
@by_set
def test_sharded_plans(name, world):
    """Plans built for worlds 2 and 4, all ranks stepped by exact_plan.run_ranks: every rank's outputs equal the reference
    (204 cases of family 1, 17 per operation, and 100 of family 3)."""
    sweep = pc.Sweep(_codec(name), world)
    for op in pc.COMPARE_OPS:
        for case in pc.family1_random(sweep.codec, op, 17, seed=2):
            sweep.check(case)
    assert sweep.cases == 204
    for case in pc.family3(sweep.codec, 100, seed=2):
        sweep.check(case)
    _report(sweep, f"world {world}")


# ---- the same names on PARAM_MESSAGE_2_CARRY_2_KS_PBS: built, and their noise books checked -------------------------

def _p22_cases(family):
    codec = _codec(P22.name)            # T = 16, msg_mod = 4 as TOY_K1: the generators yield TOY_K1's cases
    if family == 1:
        return (case for op in pc.COMPARE_OPS for gen in (pc.family1_exhaustive(codec, op), pc.family1_random(codec, op, 125)) for case in gen)
    if family == 2:
        return (case for op in pc.SHAPE_OPS for gen in (pc.family2_exhaustive(codec, op), pc.family2_random(codec, op, 91)) for case in gen)
    if family == 6:
        return (case for case, _ in pc.family6(codec, 300))
    return {3: lambda: pc.family3(codec, 3000), 4: lambda: pc.family4(codec, 600), 5: lambda: pc.family5(codec, 600)}[family]()


@pytest.mark.parametrize("family", [1, 2, 3, 4, 5, 6])
def test_noise_bookkeeping_on_p22(family):
    """Every plan name the TOY_K1 sweeps build, built on the production parameter set (budget 138.2, where replace:F:C
    reaches 130): no refusal, distinct sources in every job, max_j sum_t coeff_t^2 equal to the declared worst PBS-input
    noise and within the budget.  For programs the cleaning lookups of bind_inputs are jobs like any other."""
    import fhestr
    codec = _codec(P22.name)
    assert (codec.T, codec.M) == (_codec(O.TOY_K1.name).T, _codec(O.TOY_K1.name).M)
    seen, worst = set(), 0
    for case in _p22_cases(family):
        if case.key in seen:
            continue
        seen.add(case.key)
        try:
            plan = case.build(codec.P, 1)
        except fhestr.FheError as e:
            raise AssertionError(f"{codec.name}: plan build refused: {case.key!r}: {e}") from None
        levels = [plan.export_level(l) for l in range(plan.info()["n_levels"] + 1)]
        worst = max(worst, pc.check_noise_bookkeeping(plan, levels, f"{codec.name}: {case.key!r}"))
        plan.close()
    print(f"{codec.name} family {family}: {len(seen)} plans, worst declared noise {worst} of {fhestr.noise_model(codec.P)['budget']:.1f}")
    assert len(seen) >= 100
