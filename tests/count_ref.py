"""Clear-text definitions of the operations that take an ENCRYPTED count (repeat:<n_max>, replacen_encn,
splitn_encn, rsplitn_encn), stated with Python `bytes` on the unpadded strings.  Test infrastructure: the
tests of these operations compare against this file, never against the code under test.

The count n arrives as D little-endian base-msg_mod digits, D the smallest number with msg_mod^D > n_max
(the caller's public bound, >= 1).  A value above the bound acts as the bound: everywhere n* = min(n, n_max).

The two split forms have exactly the output layout of `splitn:<P>` with P = n_max (split_ref.decode_split
reads it): count = len(parts) in as many digits as the value P + 1 needs, then P left-justified parts."""


def input_digits(msg_mod: int, n_max: int) -> int:
    """D: how many digits the count travels in."""
    assert n_max >= 1
    d = 1
    while msg_mod ** d <= n_max:
        d += 1
    return d


def encode_count(msg_mod: int, n: int, n_max: int):
    """The D clear digits of n, little endian.  n may exceed n_max as long as D digits hold it."""
    d = input_digits(msg_mod, n_max)
    assert 0 <= n < msg_mod ** d
    return [(n // msg_mod ** i) % msg_mod for i in range(d)]


def clamp(n: int, n_max: int) -> int:
    return min(n, n_max)


def repeat_ref(a: bytes, n: int, n_max: int) -> bytes:
    return a * clamp(n, n_max)


def replacen_ref(a: bytes, frm: bytes, to: bytes, n: int, n_max: int, out_cap: int = None) -> bytes:
    """An empty encrypted `from` selects nothing (the convention of replace; a clear one is refused)."""
    k = clamp(n, n_max)
    out = a if not frm or k == 0 else a.replace(frm, to, k)      # (never bytes.replace(.., -1): "no limit")
    return out if out_cap is None else out[:out_cap]


def splitn_ref(op: str, a: bytes, sep: bytes, n: int, max_parts: int, part_cap: int = None):
    """(count, parts) of splitn_encn / rsplitn_encn: op in ("splitn", "rsplitn"), n_max = max_parts.  An empty
    encrypted separator separates nothing."""
    assert op in ("splitn", "rsplitn")
    k = clamp(n, max_parts)
    if k == 0:
        parts = []                                               # (never bytes.split(sep, -1): "no limit")
    elif not sep:
        parts = [a]
    elif op == "splitn":
        parts = a.split(sep, k - 1)
    else:
        parts = a.rsplit(sep, k - 1)[::-1]
    count = len(parts)
    assert count <= max_parts
    parts = parts + [b""] * (max_parts - count)
    if part_cap is not None:
        parts = [x[:part_cap] for x in parts]
    return count, parts
