"""Clear-text definitions of the slice family (take, skip, split_at, char_at, insert, substring), stated with Python
`bytes` on the unpadded strings, and the decoding of their outputs.  Test infrastructure: the tests of these operations
compare against this file, never against the code under test.

The position n is clear, or encrypted with a public bound n_max: a value above the bound acts as the bound
(n* = min(n, n_max); pass n_max=None for a clear position).  Positions beyond the length clamp as Python's slices do.
Every string result is cut at the output capacity C."""


def position(n: int, n_max=None) -> int:
    return n if n_max is None else min(n, n_max)


def take_ref(s: bytes, n: int, n_max=None, cap=None) -> bytes:
    return s[:position(n, n_max)][:cap]


def skip_ref(s: bytes, n: int, n_max=None, cap=None) -> bytes:
    return s[position(n, n_max):][:cap]


def split_at_ref(s: bytes, n: int, n_max=None, cap=None):
    return take_ref(s, n, n_max, cap), skip_ref(s, n, n_max, cap)


def char_at_ref(s: bytes, n: int, n_max=None):
    k = position(n, n_max)
    return int(k < len(s)), s[k:k + 1]


def insert_ref(s: bytes, n: int, t: bytes, n_max=None, cap=None) -> bytes:
    k = position(n, n_max)
    return (s[:k] + t + s[k:])[:cap]


def substring_ref(s: bytes, start: int, length: int, cap=None) -> bytes:
    return s[start:start + length][:cap]


def slice_ref(op: str, s: bytes, n: int, n_max=None, cap=None, t: bytes = b""):
    """The result of `op` as decode_slice returns it."""
    if op == "take":
        return take_ref(s, n, n_max, cap)
    if op == "skip":
        return skip_ref(s, n, n_max, cap)
    if op == "split_at":
        return split_at_ref(s, n, n_max, cap)
    if op == "char_at":
        return char_at_ref(s, n, n_max)
    assert op == "insert", op
    return insert_ref(s, n, t, n_max, cap)


def _string(msgs, msg_mod: int) -> bytes:
    bits = (msg_mod - 1).bit_length()
    bpc = 8 // bits
    msgs = [int(m) for m in msgs]
    assert len(msgs) % bpc == 0 and all(0 <= m < msg_mod for m in msgs), msgs
    chars = [sum(msgs[i + k] << (k * bits) for k in range(bpc)) for i in range(0, len(msgs), bpc)]
    text = bytes(chars).rstrip(b"\0")
    assert b"\0" not in text, chars                          # left-justified: zeros after the text and nowhere else
    return text


def decode_slice(op: str, msgs, msg_mod: int, cap: int):
    """The decrypted output blocks of a slice plan: bytes for take / skip / insert (cap characters), a pair of bytes for
    split_at (cap characters each), (bit, bytes) for char_at (cap is not read)."""
    bpc = 8 // (msg_mod - 1).bit_length()
    msgs = [int(m) for m in msgs]
    if op == "char_at":
        assert len(msgs) == 1 + bpc and msgs[0] in (0, 1), msgs
        return msgs[0], _string(msgs[1:], msg_mod)
    if op == "split_at":
        assert len(msgs) == 2 * cap * bpc, (len(msgs), cap)
        return _string(msgs[:cap * bpc], msg_mod), _string(msgs[cap * bpc:], msg_mod)
    assert len(msgs) == cap * bpc, (len(msgs), cap)
    return _string(msgs, msg_mod)
