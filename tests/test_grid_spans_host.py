"""csrc/grid_spans.h, the arithmetic behind every launch whose grid.y or grid.z grows with a batch or a key size: a count
and the device's limit for that grid dimension -> consecutive spans, one launch each.  The header is compiled on its own
with a plain host compiler into tests/grid_spans_main.cpp, plain and under AddressSanitizer + UBSan; nothing is loaded
into Python and no device is needed.  The program walks every span of every case itself (consecutive from 0, each of
1 .. limit indices, only the last one short, summing to the count); the cases below also pin the numbers the engine meets:
the batches of tests/test_gpu_batch_limits.py and the 90112 key-row quads of the two largest compact-public-key sets, under
both limits a HIP device reports for grid.y (65535 and 65536)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "grid_spans_main.cpp")
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")
BUILDS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}

# (count, limit) -> (spans, per, the spans as printed)
CASES = {
    (0, 65535): (0, 0, ""),
    (5, 0): (0, 0, ""),
    (1, 65535): (1, 1, "0+1"),
    (65535, 65535): (1, 65535, "0+65535"),
    (65536, 65535): (2, 65535, "0+65535 65535+1"),
    (65536, 65536): (1, 65536, "0+65536"),
    (65537, 65536): (2, 65536, "0+65536 65536+1"),
    (70001, 65535): (2, 65535, "0+65535 65535+4466"),
    (90112, 65535): (2, 65535, "0+65535 65535+24577"),
    (90112, 65536): (2, 65536, "0+65536 65536+24576"),
    (524280, 65535): (8, 65535, " ".join(f"{65535 * i}+65535" for i in range(8))),      # 8 x 65535: no empty ninth span
    (524281, 65535): (9, 65535, "0+65535 65535+65535 ... 458745+65535 524280+1"),
    (524280, 65536): (8, 65536, "0+65536 65536+65536 131072+65536 196608+65536 262144+65536 327680+65536 393216+65536 458752+65528"),
    (10, 3): (4, 3, "0+3 3+3 6+3 9+1"),
    (9, 3): (3, 3, "0+3 3+3 6+3"),
    (7, 1): (7, 1, "0+1 1+1 2+1 3+1 4+1 5+1 6+1"),
    (2**32 - 1, 2**31 - 1): (3, 2**31 - 1, "0+2147483647 2147483647+2147483647 4294967294+1"),
    (2**40 + 5, 2**32 - 1): (257, 2**32 - 1, None),
    (2**64 - 1, 2**32 - 1): (2**32 + 1, 2**32 - 1, None),
}
WALKED = [(c, l) for c, l in CASES if -(-c // max(l, 1)) <= 1 << 20]      # the program walks every span: keep that short


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler available")
    out = tmp_path_factory.mktemp("grid_spans")
    built = {}
    for name, flags in BUILDS.items():
        built[name] = str(out / name)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", built[name], SOURCE], check=True)
    return built


def run(program, cases):
    r = subprocess.run([program, *(f"{c},{l}" for c, l in cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * len(cases)
    return list(zip(lines[0::2], lines[1::2]))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_spans(programs, build):
    for (count, limit), (head, walk) in zip(WALKED, run(programs[build], WALKED)):
        spans, per, text = CASES[count, limit]
        assert walk == "walk: ok", (count, limit, head, walk)
        assert head.startswith(f"{count} {limit}: spans={spans} per={per}"), (count, limit, head)
        if text is not None:
            assert head == f"{count} {limit}: spans={spans} per={per}" + (" " + text if text else ""), (count, limit, head)


def test_cases_cover_what_the_engine_meets():
    assert {(c, l) for c, l in CASES if c in (65535, 65536, 65537, 70001, 90112, 524280)} >= {
        (65535, 65535), (65536, 65535), (65536, 65536), (65537, 65536), (70001, 65535), (90112, 65535), (90112, 65536),
        (524280, 65535), (524280, 65536)}
    for (count, limit), (spans, per, _) in CASES.items():
        assert spans == (-(-count // limit) if limit and count else 0) and per == (min(count, limit) if spans else 0)
