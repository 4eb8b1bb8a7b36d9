"""One line per FheString plan key and a final sha256 over all lines (CPU only; plans are built offline from `params=`).

A built key prints the sha256 of everything the plan will run: info(), noise_info(), every array of every export_level(l)
for l in 0 .. n_levels, every table of export_luts().  A refused key prints `refused: <the FheError text>`.  Two builds of
the library that print the same lines build the same plans and refuse with the same words: run it before and after a
change of the plan builder (FHESTR_LIB=/path/libfhestr.so selects the other build) and compare the outputs.

    python scripts/plan_digest.py > digest.txt
    python scripts/plan_digest.py --keys | build/sanitize/str_plans        (builds nothing itself: `make sanitize-plans`)

--keys prints the Plan.string_op keys of TOY_K1 and of the small box, one per line, in the form tests/str_plans_main.cpp reads:
the fields of fhe_params_t, world, plan name, a_cap, b_cap, the clear bytes as `x` + hex (`-`: none).

The keys:
  - every case of families 1 to 6 of tests/plan_cases.py, with the counts of tests/test_plan_sweep_cpu.py, on TOY_K1,
    TOY_N32768 and PARAM_MESSAGE_2_CARRY_2_KS_PBS, world 1 (programs too, with dedupe on and off);
  - family1_random(.., 17, seed=2) of every compare op and family3(.., 100, seed=2) at worlds 2 and 4;
  - the small box, PARAM_MESSAGE_1_CARRY_1_KS_PBS (msg_mod 2, T = 4, eight blocks per character), world 1: 17 random cases
    per compare op, 11 per shape op, 60 of family 3, 40 of family 4 -- the T < 8, T < 12 and T < 16 branches of the builder,
    most of them refusals, whose texts are hashed like everything else;
  - a refusal grid: every odd name and every step name of tests/test_program_host.py and a few more, at four capacity
    pairs and five clear operands, through Plan.string_op and through an offline StringProgram.op (the two names of
    HUGE only where they are refused before anything is built).

The output is not kept in the repository: later optimisations are meant to change plans."""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fhe-string-bounty_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import fhestr  # noqa: E402
import oracle as O  # noqa: E402
import plan_cases as pc  # noqa: E402
from test_program_host import BUILT, ODD  # noqa: E402

SETS = (O.TOY_K1, O.TOY_N32768, O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
SMALL_BOX = O.PARAM_MESSAGE_1_CARRY_1_KS_PBS
GRID_NAMES = list(ODD) + list(BUILT) + ["no_such_op", "eq_", "Eq", "matches", "matches_reference", "matches_reference_clear", "repeat", "trim",
                                        "split_ascii_whitespace_clear:2", "replacen_encn:0:1:4", "splitn_encn:0"]
GRID_CAPS = ((0, 0), (2, 0), (2, 2), (4, 3))
GRID_CLEAR = (None, b"", b"ab", b"abxy", b"/a/")
# odd names that are well formed: with a string and a pattern the builder sets out on 10^9 parts or characters.  They are
# tried only where it refuses before that (no capacity, no pattern).
HUGE = ("split_clear:999999999", "split_clear:1:999999999")


def plan_digest(plan) -> str:
    h = hashlib.sha256()
    info = plan.info()
    h.update(repr(sorted(info.items())).encode())
    h.update(repr(sorted(plan.noise_info().items())).encode())
    for l in range(info["n_levels"] + 1):
        for name, v in sorted(plan.export_level(l).items()):
            h.update(name.encode())
            h.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    for i, table in sorted(plan.export_luts().items()):
        h.update(repr(i).encode())
        h.update(np.ascontiguousarray(table).tobytes())
    return h.hexdigest()


def verdict(build) -> str:
    try:
        plan = build()
    except fhestr.FheError as e:
        return f"refused: {e}"
    try:
        return plan_digest(plan)
    finally:
        plan.close()


def sweep_cases(codec, world):
    """The cases of tests/test_plan_sweep_cpu.py for one parameter set and world."""
    if world != 1:
        for op in pc.COMPARE_OPS:
            yield from pc.family1_random(codec, op, 17, seed=2)
        yield from pc.family3(codec, 100, seed=2)
        return
    for op in pc.COMPARE_OPS:
        yield from pc.family1_exhaustive(codec, op)
        yield from pc.family1_random(codec, op, 125)
    for op in pc.SHAPE_OPS:
        yield from pc.family2_exhaustive(codec, op)
        yield from pc.family2_random(codec, op, 91)
    yield from pc.family3(codec, 1500 if codec.name == O.TOY_N32768.name else 3000)
    yield from pc.family4(codec, 600)
    yield from pc.family5(codec, 600)
    for case, _ in pc.family6(codec, 300):
        yield case


def small_box_cases(codec):
    for op in pc.COMPARE_OPS:
        yield from pc.family1_random(codec, op, 17, seed=2)
    for op in pc.SHAPE_OPS:
        yield from pc.family2_random(codec, op, 11, seed=2)
    yield from pc.family3(codec, 60, seed=2)
    yield from pc.family4(codec, 40, seed=2)


def program_plan(P, name, a_cap, b_cap, clear):
    """The op alone in an offline program, on inputs of those capacities, every result an output."""
    prog = fhestr.StringProgram(None, params=P)
    try:
        operands = [prog.string(a_cap)] + ([prog.string(b_cap)] if b_cap else [])
        prog.output(*prog.op(name, *operands, clear=clear))
        return prog.compile(1).plan
    finally:
        prog.close()


def lines():
    for params in SETS + (SMALL_BOX,):
        codec = pc.Codec(params)
        for world in (1, 2, 4) if params in SETS[:2] else (1,):
            seen = set()
            for case in small_box_cases(codec) if params is SMALL_BOX else sweep_cases(codec, world):
                if case.key in seen:
                    continue
                seen.add(case.key)
                yield f"{params.name} world {world} {case.key!r}: " + verdict(lambda: case.build(codec.P, world))
    for params in SETS[:2]:
        P = pc.Codec(params).P
        for name in GRID_NAMES:
            for a_cap, b_cap in GRID_CAPS:
                for clear in GRID_CLEAR:
                    if name in HUGE and a_cap and clear:
                        continue
                    what = f"{params.name} grid {name!r} {a_cap} {b_cap} {clear!r}"
                    yield what + " string_op: " + verdict(lambda: fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, 1, params=P))
                    yield what + " program: " + verdict(lambda: program_plan(P, name, a_cap, b_cap, clear))


def key_lines():
    for params in (O.TOY_K1, SMALL_BOX):
        codec = pc.Codec(params)
        P = codec.P
        fields = " ".join(repr(v) for v in (P.n, P.k, P.N, P.pbs_base_log, P.pbs_level, P.ks_base_log, P.ks_level, P.msg_mod,
                                            P.carry_mod, P.lwe_std, P.glwe_std, P.grouping))
        seen = set()
        for case in small_box_cases(codec) if params is SMALL_BOX else sweep_cases(codec, 1):
            if case.key[0] == "program" or case.key in seen:
                continue
            seen.add(case.key)
            name, a_cap, b_cap, clear = case.key
            yield f"{fields} 1 {name} {a_cap} {b_cap} " + ("-" if clear is None else "x" + clear.hex())


def main():
    if sys.argv[1:] == ["--keys"]:
        print("\n".join(key_lines()))
        return
    t0 = time.perf_counter()
    total, n = hashlib.sha256(), 0
    for line in lines():
        print(line)
        total.update(line.encode() + b"\n")
        n += 1
    print(f"digest {total.hexdigest()} over {n} lines")
    print(f"{time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
