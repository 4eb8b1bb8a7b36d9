#!/usr/bin/env python3
"""Times FheStringOps.matches on PARAM_MESSAGE_2_CARRY_2 (device-generated keys) next to contains_clear of a two-character
literal at the same capacities, in the same process, rounds interleaved:

  * /^[0-9]*$/ at 32 characters (one position, a loop: one lookup level per character),
  * /ab|cd/i at 64 characters (four positions, no loop: the depth of the pattern),
  * contains_clear(b"ab") at 32 and at 64 characters,

each as one call on one string, and as one pass over 8 rows (matches_many / contains_many), reported per row.  A call
is timed with the host clock around it: it uploads the string, runs the plan and downloads the result block, so it ends
in a device synchronise.  Medians over --reps calls after a warm-up, the spread over --rounds rounds beside them.

    python scripts/regex_timing.py [--out profiles/regex_matches.txt] [--reps 20] [--rounds 3]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-string-bounty_amd"))

import numpy as np  # noqa: E402

import fhestr  # noqa: E402

ROWS = 8
CASES = [("matches", b"/^[0-9]*$/", 32, b"0123456789012345678901"), ("matches", b"/ab|cd/i", 64, b"the quick brown fox jumps over the lazy dog; aCd"),
         ("contains", b"ab", 32, b"0123456789012345678901"), ("contains", b"ab", 64, b"the quick brown fox jumps over the lazy dog; aCd")]


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regex_matches.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    ck = fhestr.ClientKey(P, 0x5EED0F00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0F01)
    ops = fhestr.FheStringOps(eng)
    lines = ["matches (csrc/regex.cpp, StrOps::matches) next to contains_clear -- produced by scripts/regex_timing.py", "",
             f"{P.name}, device-generated keys; host clock around one call (upload, plan, download of the result block);",
             f"median of {args.reps} calls after warm-up, min .. max of the medians of {args.rounds} interleaved rounds; {ROWS} rows per pass", ""]
    todo = []
    for op, pat, cap, text in CASES:
        a = ck.encrypt(fhestr.string_to_blocks(P, text, cap))
        rows = np.stack([ck.encrypt(fhestr.string_to_blocks(P, text[: max(0, len(text) - r)], cap)) for r in range(ROWS)])
        name = "matches_clear" if op == "matches" else "contains_clear"
        info = fhestr.Plan.string_op(None, name, cap, 0, pat, params=P).info()
        one = (lambda a=a, pat=pat, op=op: getattr(ops, op)(a, pat))
        many = (lambda rows=rows, pat=pat, op=op: getattr(ops, op + "_many")(rows, pat))
        want = [int(ck.decrypt(x.reshape(1, -1))[0]) for x in many()]
        assert int(ck.decrypt(one().reshape(1, -1))[0]) == want[0]
        todo.append((f"{op} {pat.decode()} at {cap}", info, one, many, {"one": [], "many": []}))
    for _ in range(args.rounds):
        for _, _, one, many, got in todo:
            got["one"].append(median_ms(one, args.reps))
            got["many"].append(median_ms(many, args.reps) / ROWS)
    for label, info, _, _, got in todo:
        o, m = got["one"], got["many"]
        lines.append(f"{label:32s} {info['n_pbs']:5d} PBS {info['n_levels']:3d} levels   alone {statistics.median(o):8.2f} ms ({min(o):.2f} .. {max(o):.2f})"
                     f"   per row at {ROWS} rows {statistics.median(m):8.2f} ms ({min(m):.2f} .. {max(m):.2f})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    ops.close()
    eng.close()
    ck.close()


if __name__ == "__main__":
    main()
