"""The clear-text definition of FheStringOps.matches: the pattern text of the reference's regex engine translated to
Python's `re`, and a generator of random patterns from that grammar.

    /^?body$?/i?   ->   re.search(rb"^?(?:body)\\Z?", s, re.DOTALL [| re.I])    on the unpadded bytes

`^` and `$` exist only as the outermost anchors and bind looser than `|`, hence the group around the body; `\\x` is the
byte x itself (re.escape); everything else of the grammar reads the same in `re`."""
import re


def to_python(pattern: bytes):
    """(compiled bytes regex of `re`) of a pattern the grammar accepts."""
    assert pattern[:1] == b"/"
    icase = pattern.endswith(b"/i")
    body = pattern[1:-2] if icase else pattern[1:-1]
    assert pattern[len(body) + 1:len(body) + 2] == b"/"
    sof = body[:1] == b"^"
    if sof:
        body = body[1:]
    out, i, eof = b"", 0, False
    while i < len(body):
        ch = body[i:i + 1]
        if ch == b"\\":
            out += re.escape(body[i + 1:i + 2])
            i += 2
            continue
        if ch == b"$" and i == len(body) - 1:
            eof = True
        else:
            out += ch
        i += 1
    text = (b"^" if sof else b"") + b"(?:" + out + b")" + (b"\\Z" if eof else b"")
    return re.compile(text, re.DOTALL | (re.I if icase else 0))


def has_match(s: bytes, pattern: bytes) -> int:
    return int(to_python(pattern).search(s) is not None)


# ---- random patterns: only what the grammar accepts, at most `max_positions` character positions after expansion ----
def _atom(rng, budget, depth):
    """(text, positions)"""
    kinds = ["lit", "lit", "lit", "dot", "esc", "list", "range", "neg"] + (["group"] if depth < 2 and budget >= 2 else [])
    k = kinds[rng.integers(len(kinds))]
    if k == "lit":
        return "abc"[rng.integers(3)], 1
    if k == "dot":
        return ".", 1
    if k == "esc":
        return "\\" + "ab."[rng.integers(3)], 1
    if k == "list":
        return "[" + ["ab", "bc", "ac", "a"][rng.integers(4)] + "]", 1
    if k == "range":
        return ["[a-b]", "[b-c]", "[a-c]"][rng.integers(3)], 1
    if k == "neg":
        return ["[^a]", "[^bc]", "[^a-b]"][rng.integers(3)], 1
    text, n = _regex(rng, budget, depth + 1)
    return "(" + text + ")", n


def _factor(rng, budget, depth):
    text, n = _atom(rng, budget, depth)
    q = rng.integers(12)
    if q < 6:
        return text, n
    choices = [("?", 1), ("*", 1), ("+", 1)]
    for suffix, copies in (("{2}", 2), ("{1,}", 1), ("{2,}", 2), ("{,2}", 2), ("{1,2}", 2), ("{0}", 0), ("{,}", 1), ("{1,3}", 3)):
        if n * copies <= budget:
            choices.append((suffix, copies))
    suffix, copies = choices[rng.integers(len(choices))]
    return text + suffix, n * copies


def _term(rng, budget, depth):
    text, used = "", 0
    for _ in range(int(rng.integers(1, 4))):
        if used >= budget and text:
            break
        t, n = _factor(rng, max(1, budget - used), depth)
        if used + n > budget and text:
            break
        text, used = text + t, used + n
    return text, used


def _regex(rng, budget, depth):
    text, used = _term(rng, budget, depth)
    while used < budget and rng.integers(3) == 0:
        t, n = _term(rng, budget - used, depth)
        text, used = text + "|" + t, used + n
    return text, used


def random_pattern(rng, max_positions=6) -> bytes:
    """A random pattern /^?regex$?/i? with at most max_positions character positions after the repeats are expanded."""
    while True:
        text, used = _regex(rng, max_positions, 0)
        if used <= max_positions:
            break
    return ("/" + ("^" if rng.integers(3) == 0 else "") + text + ("$" if rng.integers(3) == 0 else "") + "/" +
            ("i" if rng.integers(4) == 0 else "")).encode()
