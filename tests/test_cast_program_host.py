"""csrc/cast.cpp on its own: the host units of casting keys -- the parameter check, cast_rshift, the follow-up table, the plain
keyswitch loop and the noise model -- compiled with a plain host compiler under AddressSanitizer + UBSan into
tests/cast_main.cpp.  The program allocates every buffer at exactly the documented size, so a one-word over-read or a word
left unwritten shows; its checksums are compared with tests/exact_cast.py here.  Nothing is loaded into Python and no
device is needed."""
import os
import subprocess
import types

import numpy as np
import pytest

from exact_cast import cast_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cast_main.cpp"), os.path.join(ROOT, "fhe-string-bounty_amd", "csrc", "cast.cpp")]
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    program = str(tmp_path_factory.mktemp("cast_main") / "cast_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-o", program, *SOURCES], check=True)
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [ln.split(" ", 1) for ln in r.stdout.split("\n")[:-1]]


def _splitmix(seed, n):
    m = np.uint64
    with np.errstate(over="ignore"):
        z = m(seed) + (np.arange(n, dtype=np.uint64) + m(1)) * m(0x9E3779B97F4A7C15)
        z = (z ^ (z >> m(30))) * m(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> m(27))) * m(0x94D049BB133111EB)
        return z ^ (z >> m(31))


def _checksum(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        return int((w * (np.arange(w.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))


def test_keyswitch_checksums_match_exact(lines):
    cases = [rest.split() for kind, rest in lines if kind == "case"]
    assert len(cases) == 8 and {int(c[3]) for c in cases} >= {1, 3, 5, 15, 16}
    for in_dim, out_dim, bl, level, target, count, got in cases:
        in_dim, out_dim, bl, level, target, count = map(int, (in_dim, out_dim, bl, level, target, count))
        seed = (in_dim << 40) ^ ((out_dim + 1) << 20) ^ (bl << 12) ^ (level << 4) ^ target
        key = _splitmix(seed, in_dim * level * (out_dim + 1))
        cts = _splitmix(~seed & (2**64 - 1), count * (in_dim + 1)).reshape(count, in_dim + 1)
        src = types.SimpleNamespace(k=1, N=in_dim)
        dst = types.SimpleNamespace(k=1, N=out_dim, n=out_dim)
        want = cast_exact(src, dst, (bl, level), target, key, cts) if count else np.zeros(0, dtype=np.uint64)
        assert int(got, 16) == _checksum(want), (in_dim, out_dim, bl, level, target, count)


def test_shifts_and_tables(lines):
    rows = [list(map(int, rest.split())) for kind, rest in lines if kind == "shift"]
    assert len(rows) == 9
    for m1, m2, shift, *table in rows:
        assert shift == m2.bit_length() - m1.bit_length()
        assert table == [x >> shift if shift > 0 else x for x in range(m2)]


def test_regrouping_rule(lines):
    """Spaces 4 (1-bit messages), 16 (2-bit) and 256 (4-bit): a regrouping passes exactly when the cast widens, msg_src^g is
    the destination's msg_mod and (msg_src^g - 1) << shift stays inside the destination's space."""
    rows = [rest.split() for kind, rest in lines if kind == "regroup"]
    assert len(rows) == 36
    msg = {4: 2, 16: 4, 256: 16}
    for m1, m2, g, got in rows:
        m1, m2, g = int(m1), int(m2), int(g)
        shift = m2.bit_length() - m1.bit_length()
        degree = (msg[m1]**g - 1) << shift if shift >= 0 else (msg[m1]**g - 1) >> -shift
        ok = g == 1 or (shift > 0 and msg[m1]**g == msg[m2] and degree < m2)
        assert got == (str(degree) if ok else "refused"), (m1, m2, g, got)
    assert ["4", "16", "2", "12"] in rows and ["16", "256", "2", "240"] in rows and ["4", "256", "4", "refused"] in rows


def test_refusals(lines):
    why = [rest for kind, rest in lines if kind == "refused"]
    assert len(why) == 10
    for got, part in zip(why, ["17 levels", "base_log 8", "base_log 0", "0 levels", "base_log * level", "target", "8053309440 bytes (limit 4 GiB)",
                               "powers of two (source 12, destination 16)", "powers of two (source 4, destination 24)", "empty source"]):
        assert part in got, (got, part)


def test_noise_lines(lines):
    rows = [list(map(float, rest.split())) for kind, rest in lines if kind == "noise"]
    assert len(rows) == 2 and rows[0][1] == rows[1][1] and rows[0][2] == rows[1][2]      # one budget, one keyswitched block
    assert rows[1][0] < rows[0][0]                                                        # TO_SMALL takes the destination's own keyswitch term off
