"""csrc/glwe_narrow.cpp on its own: the narrow form's host loops and the field reader the kernels share, compiled with a plain
host compiler under AddressSanitizer + UBSan into tests/narrow_main.cpp.  The program allocates every list at exactly
fhe_narrow_len words on the heap, so a one-word over-read is a report, runs narrow, widen and extract over the grid of
tests/test_glwe_narrow.py plus the block counts that end a stream exactly on a word boundary and one bit short of it, and
prints checksums, which are compared with tests/exact_narrow.py here.  Nothing is loaded into Python and no device is needed."""
import os
import subprocess

import numpy as np
import pytest

import exact_narrow as X
from exact_extract import RANGES, SHAPES, extract_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "narrow_main.cpp"), os.path.join(ROOT, "fhe-string-bounty_amd", "csrc", "glwe_narrow.cpp")]
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    program = str(tmp_path_factory.mktemp("narrow_main") / "narrow_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-o", program, *SOURCES], check=True)
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.split("\n")[:-1]]


def _splitmix(seed, n):
    m = np.uint64
    with np.errstate(over="ignore"):
        z = m(seed) + (np.arange(n, dtype=np.uint64) + m(1)) * m(0x9E3779B97F4A7C15)
        z = (z ^ (z >> m(30))) * m(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> m(27))) * m(0x94D049BB133111EB)
        return z ^ (z >> m(31))


def test_the_grid_is_covered(table):
    cases = {tuple(map(int, row[:4])) for row in table}
    assert len(cases) == len(table)
    for N, k in SHAPES:
        for b in X.BITS:
            held = {h for (n, kk, bb, h) in cases if (n, kk, bb) == (N, k, b)}
            assert {f(N) for f in X.HELD} <= held
            used = {((k * N + X.blocks_of(N, h, -(-h // N) - 1)) * b) % 64 for h in held - {N, 2 * N}}
            assert 0 in used and ((63 in used) == (b % 2 == 1)), (N, k, b, sorted(used))


def test_checksums_match_exact(table):
    for row in table:
        N, k, b, held = map(int, row[:4])
        got = [int(x, 16) for x in row[4:]]
        seed = (N << 40) ^ (k << 32) ^ (b << 24) ^ held
        glwes = _splitmix(seed, -(-held // N) * (k + 1) * N).reshape(-1, k + 1, N)
        narrow = X.narrow_exact(glwes, k, N, held, b)
        wide = X.widen_exact(narrow, k, N, held, b)
        want = [X.checksum(narrow), X.checksum(wide)]
        for rng_of in RANGES:
            first, count = rng_of(N)
            first = min(first, held - 1)
            count = min(count, held - first)
            want.append(X.checksum(extract_exact(wide, k, N, first, count)))
        assert got == want, (N, k, b, held)
