"""The plan builder of the names that combine results under the host sanitizers, as a stand-alone program:
tests/combine_plans_main.cpp links the planner units -- csrc/circuit.cpp, fhe_string.cpp and the str_*.cpp units behind
str_ops.h; the count arithmetic (count_ops.h) and the radix code it shares with the integer plans (radix_ops.h) are headers
-- compiled with a plain host compiler under AddressSanitizer + UBSan, and builds every new name offline at capacities and
bounds 1 .. 9, the count names also at three-digit bounds (encrypted and clear second operands, one and two ranks, 2-bit
and 4-bit blocks).  Nothing is loaded into Python and no device is needed: the engine's device calls are stubs the program
never reaches."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fhe-string-bounty_amd", "csrc")
UNITS = ["circuit.cpp", "fhe_string.cpp", "str_ops.cpp", "str_match.cpp", "str_replace.cpp", "str_split.cpp", "str_slice.cpp",
         "str_regex_match.cpp", "regex.cpp", "str_op_name.cpp"]
SOURCES = [os.path.join(ROOT, "tests", "combine_plans_main.cpp")] + [os.path.join(CSRC, u) for u in UNITS]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
COMPILERS = (os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    out = tmp_path_factory.mktemp("combine_plans_main")
    objects = [str(out / (os.path.basename(s) + ".o")) for s in SOURCES]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:      # one compiler process per unit
        for r in pool.map(lambda so: subprocess.run([cxx, *FLAGS, "-c", "-o", so[1], so[0]], capture_output=True, text=True), zip(SOURCES, objects)):
            assert r.returncode == 0, r.stderr[-3000:]
    program = str(out / "combine_plans_main")
    # the HIP runtime resolves the device-buffer calls of circuit.cpp; no call of it is reached
    subprocess.run([cxx, "-fsanitize=address,undefined", "-o", program, *objects, "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROCM, "lib")], check=True)
    return subprocess.run([program], capture_output=True, text=True, timeout=300)


def test_every_combining_name_builds_at_bounds_1_to_9_and_the_sanitizers_stay_silent(report):
    assert report.returncode == 0 and report.stderr == "", (report.returncode, report.stdout[-2000:], report.stderr[-3000:])
    lines = report.stdout.split("\n")
    built, refused = (int(w) for w in lines[-2].replace(" built,", "").replace(" refused", "").split())
    # per parameter set and world: bit logic 4 x 9, select 9 x 3 x (2 + 2), select_count 81, the count names 8 x (81 + 9 x 5) and
    # at eight larger bounds 8 x 8 x (4 + 2); refused: and / or / xor at k = 1
    per = 4 * 9 + 9 * 3 * 4 + 81 + 8 * (81 + 45) + 8 * 8 * 6
    assert (built + refused, refused) == (2 * 2 * per, 2 * 2 * 3), (built, refused)
    assert len(lines) - 2 == built + refused                 # one line per plan: its info, or the refusal
    assert sum("\trefused\t" in ln and "k must be at least 2" in ln for ln in lines) == refused
