"""Instruction budget of the P22 CMUX step (no GPU needed).

Compiles csrc/blind_rotate.hip to gfx950 assembly the way scripts/isa_load_waits.py does, takes the main loop of
blind_rotate_wide_kernel<11,2,2,1,false> (PARAM_MESSAGE_2_CARRY_2's kernel, the one bench.py's headline spends its
time in) and checks its per-wave-step instruction counts against the budget of kernel revision r04.2, so that a
register-allocation or scheduling change that quietly brings back instructions is seen here:

  group                                   r04.1   r04.2
  VALU, all                               1,045     965
  f64 (add, fma, mul, fract)                656     656
  integer (VALU that is neither f64, a permlane swap nor a conversion)
                                            261     181
  LDS instructions                          145     137   (the 16 gather reads issued together: 8 ds_read2st64_b64)
  s_waitcnt lgkmcnt(0) before the first digit conversion
                                             16       1

plus zero scratch and at most 256 VGPRs (two workgroups per CU: pipeline mode 2 depends on it)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "_ZN3fhe24blind_rotate_wide_kernelILi11ELi2ELi2ELi1ELb0EEEvNS_15BlindRotateArgsE"

BUDGET = {"valu": 965, "f64": 656, "int": 181}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "engine.s")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                    "-ffp-contract=off", "--cuda-device-only", "-S", "-o", out,
                    os.path.join(ROOT, "fhe-string-bounty_amd", "csrc", "blind_rotate.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_lines(text):
    lines, inside = [], False
    for l in text.splitlines():
        if l.startswith(KERNEL + ":"):
            inside = True
            continue
        if inside:
            lines.append(l)
            if "s_endpgm" in l:
                break
    assert lines, "kernel not found in the assembly"
    return [l for l in lines if not l.strip().startswith(";")]


def main_loop(lines):
    """The largest backward branch's body: the per-CMUX-step loop."""
    labels = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", l)}
    best = None
    for i, l in enumerate(lines):
        m = re.search(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and (best is None or i - labels[m.group(1)] > best[0]):
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    assert best, "no loop found"
    return lines[best[1]:best[2] + 1]


def loop_counts(lines):
    c = {"valu": 0, "f64": 0, "int": 0, "swap": 0, "cvt": 0, "gather_drains": 0}
    before_digits = True
    for l in main_loop(lines):
        t = l.strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_cvt_f64"):
            before_digits = False
        if before_digits and op == "s_waitcnt" and "lgkmcnt(0)" in t:
            c["gather_drains"] += 1
        if not op.startswith("v_"):
            continue
        c["valu"] += 1
        if "permlane" in op:
            c["swap"] += 1
        elif op.startswith("v_cvt"):
            c["cvt"] += 1
        elif "f64" in op:
            c["f64"] += 1
        else:
            c["int"] += 1
    return c


def test_cmux_step_instruction_budget(asm):
    c = loop_counts(kernel_lines(asm))
    for k, limit in BUDGET.items():
        assert c[k] <= limit, f"{k}: {c[k]} instructions per wave-step, budget {limit} ({c})"


def test_gather_reads_are_not_serialised(asm):
    """The rotation gather's LDS reads are all in flight before the first is used: one full drain of the LDS queue
    before the digits are converted, not one per read (16 round trips of ~130 cycles per wave-step)."""
    c = loop_counts(kernel_lines(asm))
    assert c["gather_drains"] <= 2, c


def test_no_scratch_and_two_workgroups_per_cu(asm):
    vgpr = int(re.search(r"\.set " + re.escape(KERNEL) + r"\.num_vgpr, (\d+)", asm).group(1))
    scratch = int(re.search(r"\.set " + re.escape(KERNEL) + r"\.private_seg_size, (\d+)", asm).group(1))
    assert scratch == 0
    assert vgpr <= 256
