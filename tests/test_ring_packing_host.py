"""csrc/ring_packing.cpp on its own: the parameter check, the host transform and the host reference of ring packing,
compiled with a plain host compiler under AddressSanitizer + UBSan into tests/ring_packing_main.cpp.  The program allocates
every buffer at exactly its length on the heap, packs splitmix64 keys and LWEs over the shapes and counts of
tests/test_ring_packing.py, and prints checksums, which are compared with tests/exact_ring_packing.py here; it also runs
the transform's round trips and the all-extreme product at the one-prime bound.  Nothing is loaded into Python and no
device is needed."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import exact_ring_packing as X
from exact_narrow import checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "ring_packing_main.cpp"), os.path.join(ROOT, "fhe-string-bounty_amd", "csrc", "ring_packing.cpp")]
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")
SHAPES = [(16, 1, 8, 4), (16, 1, 3, 7), (64, 1, 6, 4), (16, 2, 5, 3), (8, 3, 4, 5), (8, 3, 10, 2)]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    program = str(tmp_path_factory.mktemp("ring_packing_main") / "ring_packing_main")
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


def test_the_grid_is_covered(lines):
    cases = {tuple(map(int, row[:5])) for row in lines if row[0] != "transform"}
    assert cases == {(N, k, b, L, c) for (N, k, b, L) in SHAPES for c in (1, 2, 3, N - 1, N, N + 1)}
    assert [row for row in lines if row[0] == "transform"] == [["transform", str(N), "ok"] for N in (4, 64, 2048, 32768)]


def test_checksums_match_the_definition(lines):
    for row in lines:
        if row[0] == "transform":
            continue
        N, k, b, L, count = map(int, row[:5])
        seed = (N << 40) ^ (k << 32) ^ (b << 24) ^ (L << 16) ^ count
        key = _splitmix(seed, (N.bit_length() - 1) * k * L * (k + 1) * N)
        cts = _splitmix(seed ^ 0x5555555555555555, count * (k * N + 1))
        want = X.ring_pack_int(SimpleNamespace(k=k, N=N), (b, L), key, cts)
        assert int(row[5], 16) == checksum(want), (N, k, b, L, count)
