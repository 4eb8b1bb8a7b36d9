"""csrc/regex.cpp on its own: the pattern parser and automaton construction of matches_clear, compiled with a plain host
compiler under AddressSanitizer + UBSan into tests/regex_main.cpp, which feeds it a valid corpus, malformed and truncated
patterns, every prefix of a few valid patterns, deep nesting and huge repeat counts, and prints one line per pattern.
Nothing is loaded into Python and no device is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "regex_main.cpp"), os.path.join(ROOT, "fhe-string-bounty_amd", "csrc", "regex.cpp")]
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")

# pattern as printed -> (positions, max_len, literal)
VALID = {
    "/h/": (1, "1", "h"), "/&/": (1, "1", "&"), "/\\\\h/": (1, "1", "h"), "/./": (1, "1", "-"), "/abc/": (3, "3", "abc"),
    "/^abc/": (3, "3", "abc"), "/abc$/": (3, "3", "abc"), "/^abc$/": (3, "3", "abc"), "/^ab?c$/": (3, "3", "-"),
    "/^ab*c$/": (3, "inf", "-"), "/^ab+c$/": (3, "inf", "-"), "/^ab{2}c$/": (4, "4", "abbc"), "/^ab{3,}c$/": (5, "inf", "-"),
    "/^ab{2,4}c$/": (6, "6", "-"), "/^ab{,4}c$/": (6, "6", "-"), "/^.$/": (1, "1", "-"), "/^[abc]$/": (1, "1", "-"),
    "/^[a-d]$/": (1, "1", "-"), "/^[^abc]$/": (1, "1", "-"), "/^[^a-d]$/": (1, "1", "-"), "/^abc$/i": (3, "3", "-"),
    "/^a(bc)d$/": (4, "4", "abcd"), "/ab|cd/": (4, "2", "-"), "/^ab|cd|de$/": (6, "2", "-"), "/^[0-9]*$/": (1, "inf", "-"),
    "/[a-z]+@[a-z]+/": (3, "inf", "-"), "/ab|cd/i": (4, "2", "-"), "/[a-c]/i": (1, "1", "-"), "/\\\\//": (1, "1", "/"),
    "/\\\\\\\\/": (1, "1", "\\\\"), "/^$/": (0, "0", "-"), "/^/": (0, "0", "-"), "/$/": (0, "0", "-"), "/a{0}/": (0, "0", "-"),
    "/a{,}/": (1, "inf", "-"), "/(a{0}){999999999}/": (0, "0", "-"), "/(a|b)*abb/": (5, "inf", "-"),
    "/((a|b)?c){2,3}$/": (9, "6", "-"), "/[^^a]/": (1, "1", "a"), "/(a{16}){16}/": (256, "256", "a" * 256),
    "/a{256}/": (256, "256", "a" * 256), "/(a?){256}/": (256, "256", "-"), "/x(a|b|c|d|e|f|g|h|i|j)k/": (12, "3", "-"),
    "/(a)/": (1, "1", "a"), "/((((((((a))))))))/": (1, "1", "a"), "/" + "(" * 64 + "a" + ")" * 64 + "/": (1, "1", "a"),
    "/" + "a" * 256 + "/": (256, "256", "a" * 256), "/a" + "|a" * 255 + "/": (256, "1", "-"),
    "/^(ab|c[d-f]+){2,3}\\\\.x*$/": (14, "inf", "-"), "/^(ab|c[d-f]+){2,3}\\\\.x*$/i": (14, "inf", "-"),
    "/[^a-c]?(x|yz{,2})+@[0-9]{2}/": (8, "inf", "-"), "/((a|b)(c|d)){2}e{1,}/": (9, "inf", "-"),
}
# pattern as printed -> what the reason names
REFUSED = {
    "": "at byte 0", "/": "at byte 1: missing the closing /", "//": "at byte 1: empty pattern", "a": "at byte 0", "/a": "at byte 2: missing the closing /",
    "/a/x": "at byte 3", "/a/ii": "at byte 4", "/a**/": "at byte 3", "/*a/": "at byte 1: a repeat with nothing to repeat",
    "/+/": "at byte 1", "/?/": "at byte 1", "/{2}/": "at byte 1", "/a{}/": "at byte 2: empty repeat count {}",
    "/a{3,2}/": "at byte 2: repeat count {n,m} with n > m", "/a{2/": "at byte 4", "/a{2,/": "at byte 5", "/a{x}/": "at byte 3",
    "/a{2,3,4}/": "at byte 6", "/a|/": "at byte 3: empty alternative", "/|a/": "at byte 1: empty alternative",
    "/a||b/": "at byte 3: empty alternative", "/()/": "at byte 2: empty group", "/(|a)/": "at byte 2: empty alternative",
    "/(a/": "at byte 3", "/a)/": "at byte 2: unbalanced )", "/)/": "at byte 1: unbalanced )", "/[/": "at byte 2", "/[]/": "at byte 2: empty class",
    "/[a/": "at byte 3", "/[a-]/": "at byte 3", "/[-a]/": "at byte 2", "/[a-zA]/": "at byte 5", "/[z-a]/": "at byte 2: class range out of order",
    "/[^]/": "at byte 3: empty class", "/[a.]/": "at byte 3", "/\\\\": "at byte 1: escape at the end", "/a\\\\": "at byte 2: escape at the end",
    "/a$b/": "at byte 3", "/a^b/": "at byte 2", "/^^a/": "at byte 2", "/a$$/": "at byte 3", "/a\\x20b/": "at byte 2", "/a=b/": "at byte 2",
    "/<a>/": "at byte 1", "/a{999999999}/": "more than 256 automaton positions", "/a{99999999999999999999}/": "more than 256 automaton positions",
    "/a{257}/": "more than 256 automaton positions", "/(a{16}){17}/": "more than 256 automaton positions",
    "/((a{200}){200}){200}/": "more than 256 automaton positions", "/(a+){300}/": "more than 256 automaton positions",
    "/a{1,999999999}/": "more than 256 automaton positions", "/a\\x00b/": "at byte 2: a NUL byte", "/caf\\xc3\\xa9/": "non-ASCII byte at offset 4",
    "/\\xff/": "non-ASCII byte at offset 1", "/[\\x80]/": "non-ASCII byte at offset 2", "/\\\\\\xe9/": "non-ASCII byte at offset 2",
    "/" + "a" * 257 + "/": "more than 256 automaton positions", "/a" + "|a" * 256 + "/": "more than 256 automaton positions",
    "/((((((((a/": "at byte 10", "/a))))))))/": "at byte 2: unbalanced )",
}
for depth in (65, 1000, 100000):
    REFUSED["/" + "(" * depth + "a" + ")" * depth + "/"] = "at byte 65: groups nested too deeply"
    REFUSED["/" + "(" * depth + "a/"] = "at byte 65: groups nested too deeply"
for depth in (64, 65, 1000, 100000):
    REFUSED["/a" + ")" * depth + "/"] = "at byte 2: unbalanced )"
REFUSED["/" + "(" * 64 + "a/"] = "at byte 66"
PREFIXED = ["/^(ab|c[d-f]+){2,3}\\\\.x*$/i", "/[^a-c]?(x|yz{,2})+@[0-9]{2}/", "/((a|b)(c|d)){2}e{1,}/"]       # as printed


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    program = str(tmp_path_factory.mktemp("regex_main") / "regex_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-o", program, *SOURCES], check=True)
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [ln.split("\t") for ln in r.stdout.split("\n")[:-1]]


def test_every_line_is_a_verdict(table):
    for row in table:
        assert (row[1] == "ok" and len(row) == 5) or (row[1] == "refused" and len(row) == 3 and row[2]), row[:3]


def test_valid_corpus(table):
    got = {row[0]: (int(row[2]), row[3], row[4]) for row in table if row[1] == "ok"}
    assert got == VALID


def test_malformed_patterns_are_refused_with_the_offset(table):
    got = {row[0]: row[2] for row in table if row[1] == "refused"}
    for pattern, reason in REFUSED.items():
        assert reason in got[pattern], (pattern[:60], got[pattern])
        assert got[pattern].startswith(("malformed pattern at byte ", "non-ASCII byte at offset ", "pattern expands to more than 256"))


def test_every_prefix_of_a_valid_pattern_has_a_verdict(table):
    verdict = {row[0]: row[1] for row in table}
    for full in PREFIXED:
        assert verdict[full] == "ok"
        raw = full.replace("\\\\", "\\")
        for n in range(len(raw)):
            shown = raw[:n].replace("\\", "\\\\")
            assert shown in verdict, shown
            if shown not in VALID:
                assert verdict[shown] == "refused", shown
    assert len(table) == 43 + 56 + sum(len(p.replace("\\\\", "\\")) + 1 for p in PREFIXED) + 18 + 4
