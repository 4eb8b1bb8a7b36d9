"""The calls of the FheString Python surface that tests/test_string_calls_cpu.py resolves: every public operation over
small capacities and every form of its operands.  A call is (method name, operands, keyword arguments); an operand is
described, not given: ("s", cap) an encrypted string of that capacity, bytes a clear pattern, ("n", n_max) an encrypted
count with that public bound, an int a clear count, None an operand the method does not take.  operands_for_ops /
operands_for_program turn the descriptions into what FheStringOps / StringProgram take."""
import numpy as np

CAPS = (1, 4, 5)
BINARY = ("eq", "ne", "starts_with", "ends_with", "contains", "find", "rfind", "eq_ignore_case", "lt", "le", "gt", "ge",
          "concat", "strip_prefix", "strip_suffix")
UNARY = ("len", "is_empty", "to_upper", "to_lower", "trim_start", "trim_end", "strip")
SPLITS = ("split", "rsplit", "split_terminator", "rsplit_terminator", "split_inclusive", "splitn", "rsplitn")
ONCE = ("split_once", "rsplit_once")
N_MAX = (1, 3, 5)


def _from_to():
    """from / to: clear of equal and different lengths, an empty `to`, an empty `from`; encrypted of equal and different
    capacities and a `to` of capacity 0."""
    yield from ((b"ab", b"cd"), (b"ab", b"c"), (b"a", b""), (b"", b"x"))
    yield from ((("s", f), ("s", t)) for f, t in ((1, 1), (4, 4), (4, 1), (1, 5), (4, 0)))


def _out_caps(a_cap):
    """absent, smaller, larger"""
    return [None] + ([a_cap - 1] if a_cap > 1 else []) + [a_cap + 2]


def grid():
    for a_cap in CAPS:
        a = ("s", a_cap)
        for op in BINARY:
            for b in [("s", c) for c in CAPS] + [b"ab", b""]:
                yield op, (a, b), {}
        yield "matches", (a, "/ab|c/"), {}
        for op in UNARY:
            yield op, (a,), {}
        for frm, to in _from_to():
            for out_cap in _out_caps(a_cap):
                yield "replace", (a, frm, to), {"out_cap": out_cap}
                for n in (0, 1, 3) + tuple(("n", m) for m in N_MAX):
                    yield "replacen", (a, frm, to, n), {"out_cap": out_cap}
        for count in (0, 1, 3, 256) + tuple(("n", m) for m in N_MAX):       # (255 copies build for half a minute)
            yield "repeat", (a, count), {}
        for part_cap in (None, 1, 5):
            for pat in (("s", 1), ("s", 4), b",", b""):
                for op in SPLITS:
                    for max_parts in (1, 2, 3) + (tuple(("n", m) for m in N_MAX) if op in ("splitn", "rsplitn", "split") else ()):
                        yield op, (a, pat, max_parts), {"part_cap": part_cap}
                for op in ONCE:
                    yield op, (a, pat), {"part_cap": part_cap}
            for max_parts in (1, 2, 3):
                yield "split_ascii_whitespace", (a, max_parts), {"part_cap": part_cap}
        yield "split", (a, b",", 2), {"part_cap": 0}


def operands_for_ops(fhestr, params, operands):
    """Zero ciphertexts of the right shapes: resolving a call looks at shapes only."""
    bpc = fhestr.blocks_per_char(params)

    def one(x):
        if isinstance(x, tuple) and x[0] == "s":
            return np.zeros((x[1] * bpc, params.big_size), dtype=np.uint64)
        if isinstance(x, tuple):
            return fhestr.EncryptedCount(np.zeros((fhestr.count_input_digits(params, x[1]), params.big_size), dtype=np.uint64), x[1])
        return x

    return [one(x) for x in operands]


def operands_for_program(prog, operands):
    return [(prog.string(x[1]) if x[0] == "s" else prog.count(x[1])) if isinstance(x, tuple) else x for x in operands]
