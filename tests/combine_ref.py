"""Clear-text definitions of the plan names that combine results -- bit logic, select, arithmetic and comparisons on counts
-- and the decoding of their outputs.  Test infrastructure: the tests of these names compare against this file, never
against the code under test.

A count arrives as D little-endian base-msg_mod digits, D the smallest number with msg_mod^D > n_max (count_ref.py).  The
count_ names apply the clamping of the _encn names: an operand above its bound acts as the bound, so they are defined on
a* = min(a, a_max) and b* = min(b, b_max).  select_count passes the chosen digits through."""
import functools
import operator

from count_ref import input_digits

COMPARISONS = {"eq": operator.eq, "ne": operator.ne, "lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge}
COUNT_OPS = ("add", "sub") + tuple(COMPARISONS)


def bits_ref(op: str, bits):
    """and / or / xor: one bit; not: every bit negated."""
    if op == "not":
        return [1 - b for b in bits]
    return functools.reduce({"and": operator.and_, "or": operator.or_, "xor": operator.xor}[op], bits)


def fit_ref(s: bytes, cap: int) -> bytes:
    """Cut to cap characters (zero padding does not show on unpadded bytes)."""
    return s[:cap]


def select_ref(c: int, a: bytes, b: bytes, cap: int) -> bytes:
    return fit_ref(a if c else b, cap)


def select_count_ref(c: int, a: int, b: int) -> int:
    return a if c else b


def count_ref(op: str, a: int, a_max: int, b: int, b_max=None):
    """count_<op> on a with the bound a_max and b with the bound b_max (None: b is the clear integer).  add and sub give a
    number, the comparisons a bit."""
    a, b = min(a, a_max), b if b_max is None else min(b, b_max)
    if op == "add":
        return a + b
    if op == "sub":
        return max(a - b, 0)
    return int(COMPARISONS[op](a, b))


def count_bound(op: str, a_max: int, b_max_or_clear: int) -> int:
    """The public bound of the result of count_add / count_sub."""
    return a_max + b_max_or_clear if op == "add" else a_max


def clear_bytes(k: int) -> bytes:
    """The clear integer of a _clear count name: as few little-endian bytes as hold it, at least one."""
    return k.to_bytes(max(1, (k.bit_length() + 7) // 8), "little")


def decode_digits(msgs, msg_mod: int, n_max: int) -> int:
    """A count result: exactly the digits its bound needs, each a clean digit."""
    msgs = [int(m) for m in msgs]
    assert len(msgs) == input_digits(msg_mod, n_max), (msgs, n_max)
    assert all(0 <= m < msg_mod for m in msgs), msgs
    return sum(m * msg_mod ** i for i, m in enumerate(msgs))


def decode_bit(msgs) -> int:
    msgs = [int(m) for m in msgs]
    assert len(msgs) == 1 and msgs[0] in (0, 1), msgs
    return msgs[0]


def decode_string(msgs, msg_mod: int, cap: int) -> bytes:
    """A string of cap characters, little-endian blocks per character, zero padded and left-justified."""
    bits = msg_mod.bit_length() - 1
    bpc = 8 // bits
    msgs = [int(m) for m in msgs]
    assert len(msgs) == cap * bpc and all(0 <= m < msg_mod for m in msgs), (len(msgs), cap)
    chars = bytes(sum(msgs[i * bpc + k] << (k * bits) for k in range(bpc)) for i in range(cap))
    text = chars.rstrip(b"\0")
    assert b"\0" not in text, chars
    return text
