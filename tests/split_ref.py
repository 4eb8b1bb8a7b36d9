"""Clear-text definitions of the split family and replacen (Rust's `str` methods, stated with Python
`bytes`), and the decoder of the operations' output layout.  Test infrastructure: the tests of these
operations compare against this file, never against the code under test.

Output layout of a split plan: the count digits (little-endian base msg_mod, as many as max_parts + 1
needs; split_once / rsplit_once: ONE found block instead), then max_parts parts of part_cap characters,
left-justified and zero padded."""

ONCE = ("split_once", "rsplit_once")
SPLIT_OPS = ("split", "rsplit", "split_terminator", "rsplit_terminator", "split_inclusive", "splitn", "rsplitn",
             "split_once", "rsplit_once")


def split_parts(op: str, s: bytes, sep: bytes = None, n: int = None):
    """All parts of `op`, in the order Rust yields them (split_once / rsplit_once: (found, [before, after]))."""
    if op == "split_ascii_whitespace":
        return s.split()
    assert sep, "the separator is non-empty"
    if op == "split":
        return s.split(sep)
    if op == "rsplit":
        return s.rsplit(sep)[::-1]
    if op == "split_terminator":
        q = s.split(sep)
        return q[:-1] if q[-1] == b"" else q
    if op == "rsplit_terminator":
        q = s.rsplit(sep)[::-1]
        return q[1:] if q[0] == b"" else q
    if op == "split_inclusive":
        q = s.split(sep)
        return [x + sep for x in q[:-1]] + ([q[-1]] if q[-1] else [])
    if op == "splitn":
        return s.split(sep, n - 1)
    if op == "rsplitn":
        return s.rsplit(sep, n - 1)[::-1]
    if op == "split_once":
        before, f, after = s.partition(sep)
        return bool(f), [before, after]
    if op == "rsplit_once":
        before, f, after = s.rpartition(sep)
        return bool(f), [before, after]
    raise ValueError(op)


def split_ref(op: str, s: bytes, sep: bytes = None, max_parts: int = None, n: int = None, part_cap: int = None):
    """(count, parts) as a plan with these parameters reports them: count = min(number of parts, max_parts + 1)
    (found, as 0/1, for split_once / rsplit_once), parts = exactly max_parts strings (missing ones empty, further ones
    dropped), each cut to part_cap characters.  For splitn / rsplitn max_parts is n."""
    if op in ONCE:
        found, parts = split_parts(op, s, sep)
        count, max_parts = int(found), 2
    else:
        if op in ("splitn", "rsplitn"):
            max_parts = n = n if n is not None else max_parts
        parts = split_parts(op, s, sep, n)
        count = min(len(parts), max_parts + 1)
    parts = (list(parts) + [b""] * max_parts)[:max_parts]
    if part_cap is not None:
        parts = [x[:part_cap] for x in parts]
    return count, parts


def count_digits(msg_mod: int, max_parts: int) -> int:
    d = 1
    while msg_mod ** d <= max_parts + 1:
        d += 1
    return d


def decode_split(op: str, msgs, msg_mod: int, max_parts: int, part_cap: int):
    """(count, parts) from the decrypted output blocks of a split plan."""
    msgs = [int(m) for m in msgs]
    bits = msg_mod.bit_length() - 1
    bpc = 8 // bits
    if op in ONCE:
        n_dig, max_parts = 1, 2
    else:
        n_dig = count_digits(msg_mod, max_parts)
    assert len(msgs) == n_dig + max_parts * part_cap * bpc, (len(msgs), n_dig, max_parts, part_cap)
    count = sum(d * msg_mod ** i for i, d in enumerate(msgs[:n_dig]))
    parts = []
    for p in range(max_parts):
        blocks = msgs[n_dig + p * part_cap * bpc: n_dig + (p + 1) * part_cap * bpc]
        chars = bytes(sum(blocks[i * bpc + k] << (bits * k) for k in range(bpc)) for i in range(part_cap))
        assert b"\0" not in chars.rstrip(b"\0"), ("a part is left-justified and zero padded", chars)
        parts.append(chars.rstrip(b"\0"))
    return count, parts
