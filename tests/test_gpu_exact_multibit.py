"""Multi-bit blind rotation against exact integers at every batch regime (tier 1 of tests/test_gpu_exact_rotation.py:
the whole output ciphertext, mask and body, equals multi_bit_pbs_exact_batch bit for bit under a structured key).

What the batch size changes (choose_rotate_path, rotate_multibit_combined, rotate_multibit_two_kernel in csrc/blind_rotate.hip):
    N = 2048, B <= multibit_combine_max = 64   multibit_combine_kernel walks chunks of 8 LWEs (grid z = ceil(B / 8)), then the
                                               PRE rotation reads [B][n/G] prepared GGSWs: B = 1, 7, 8, 9, 17, 64
    N = 2048, B > 64                           the fused kernel, one workgroup per LWE and no two-per-CU twin: 65, 256 (the
                                               benchmark's launch), 257 and 515 (more workgroups than the 256 CUs)
    either kernel on the other side of 64      set_multibit_combine_max(0) at B = 64, (1024) at B = 65
    every other shape                          generic combine (grid z = ceil(sub / 8)) + the classic kernel's EXTPROD mode, in
                                               sub-batches of sub_max LWEs: lwe_small, lut_idx, lwe_out advance by `first`, the N = 8192
                                               rotation workspace lies behind sub_max prepared LWEs
sub_max follows free memory, so on an idle MI355X one sub-batch holds any test's batch; FHESTR_MULTIBIT_WS_CAP (bytes, read
when an engine is created) sets the cap, and the tests choose it so that sub_max is 3 and 5: neither divides DISTINCT, so
a sub-batch that started from the wrong LWE, table index or output row cannot land on an identical tiled slot.
Real n (818, 888 at N = 2048; 765 at N = 512, k = 3): hundreds of groups, the degree table in dynamic LDS, the
prefetch over hundreds of steps.  The real N = 8192 sets (n = 922, 972) are left out: drawing the structured key of n = 922
(0.9 GB, and as much again for the reference's integer copy) takes 2.4 s on the CPU and the numpy reference 2.5 s for ONE
LWE, before the key is converted on the GPU -- several times what a case of this suite may cost.

The reference of a shape (DISTINCT pairs, or 3 for real n) is computed once and shared, read-only, by all of its cases: a
rig's key, tables and inputs follow from the shape's seed alone."""
import numpy as np
import pytest

import oracle as O
from test_gpu_exact_rotation import DISTINCT, MB_N2048, MB_OTHER, _assert_exact, _Exact

pytestmark = pytest.mark.gpu

WS_CAP = "FHESTR_MULTIBIT_WS_CAP"
_REF = {}


def _pairs(e, distinct=DISTINCT):
    """`distinct` (ciphertext, table choice) pairs of the rig's shape and their exact outputs: the rig's own inputs(distinct),
    drawn first thing after creation, kept per shape."""
    key = (e.p.name, e.G, distinct)
    if key not in _REF:
        cts, sel, want = e.inputs(distinct)
        for a in (cts, sel, want):
            a.setflags(write=False)
        _REF[key] = (cts, sel, want, e.luts.copy())
    cts, sel, want, luts = _REF[key]
    assert np.array_equal(luts, e.luts)              # same seed: the same stream gave this rig's key and tables
    return cts, sel, want


def _check(e, B, distinct=DISTINCT, what=""):
    cts, sel, want = _pairs(e, distinct)
    slots = np.arange(B) % len(cts)
    got = e.eng.pbs(cts[slots], e.ids[sel[slots]])
    try:
        _assert_exact(got, want[slots])
    except AssertionError as err:
        raise AssertionError(f"{e.p.name}, B = {B}{what}: {err}") from None


def _run(p, G, B, setup=None, distinct=DISTINCT):
    e = _Exact(p, G)
    try:
        if setup:
            setup(e.eng)
        for b in np.atleast_1d(B):
            _check(e, int(b), distinct)
    finally:
        e.close()


def _ids(shapes):
    return [p.name for p, _ in shapes]


# ---- N = 2048: the combined prepass, the switch at 64, the fused kernel ------------------------------------------------

@pytest.mark.parametrize("p,G", MB_N2048, ids=_ids(MB_N2048))
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17, 64], ids=lambda b: f"B{b}")
def test_n2048_combined_prepass(p, G, B):
    """One partial chunk, a full one, the 8 -> 9 boundary, several chunks, the largest batch of the default threshold."""
    _run(p, G, B)


@pytest.mark.parametrize("p,G", MB_N2048, ids=_ids(MB_N2048))
@pytest.mark.parametrize("B", [65, 256, 257, 515], ids=lambda b: f"B{b}")
def test_n2048_fused_kernel(p, G, B):
    """First batch past the threshold, the benchmark's 256, and grids that run in waves over the 256 CUs."""
    _run(p, G, B)


@pytest.mark.parametrize("p,G", MB_N2048, ids=_ids(MB_N2048))
@pytest.mark.parametrize("B,combine_max", [(64, 0), (65, 1024)], ids=["B64_fused", "B65_prepass"])
def test_n2048_threshold_on_the_other_kernel(p, G, B, combine_max):
    """Both kernels are right at both sides of 64, not merely equal to each other."""
    _run(p, G, B, setup=lambda eng: eng.set_multibit_combine_max(combine_max))


# ---- the two-kernel path, whole-call batches -----------------------------------------------------------------------------

LDS_RESIDENT = [(p, G) for p, G in MB_OTHER if p.N <= 256]
WHOLE = [(p, G, B) for p, G in MB_OTHER for B in (1, 8, 9, 70)] + [(p, G, 257) for p, G in LDS_RESIDENT]


@pytest.mark.parametrize("p,G,B", WHOLE, ids=[f"{p.name}-B{B}" for p, _, B in WHOLE])
def test_two_kernel_whole_call(p, G, B):
    """One sub-batch (the automatic cap): the generic combine's chunks of 8, and 70 / 257 rotation workgroups."""
    assert len(LDS_RESIDENT) == 4
    _run(p, G, B)


# ---- the two-kernel path in forced sub-batches ----------------------------------------------------------------------------

SPLIT = [(O.TOY_MULTI_BIT_N256, 2), (O.TOY_MULTI_BIT_N256_G3, 3), (O.TOY_MULTI_BIT_N128_K2, 2), (O.TOY_MULTI_BIT_N512_K3_G3, 3),
         (O.TOY_MULTI_BIT_N8192, 2), (O.TOY_MULTI_BIT_N8192_G3, 3)]


def _per_lwe_bytes(p, G):
    """What rotate_multibit_two_kernel keeps per LWE of a sub-batch: n / G prepared GGSWs of L (k+1)^2 N/2 c64 each, and
    for N = 8192 the rotation workspace (pbs_seq_kernels.hip.h: the accumulator's k polynomials beyond the one in LDS)."""
    combined = p.pbs_level * (p.k + 1) ** 2 * (p.N // 2) * 16
    rot_ws = p.k * p.N * 8 if p.N == 8192 else 0
    return p.n // G * combined + rot_ws


def _cap_for(p, G, sub_max):
    """A cap in bytes under which the engine's sub_max = cap / per-LWE bytes comes out as `sub_max` (and is no multiple of the unit)."""
    unit = _per_lwe_bytes(p, G)
    cap = sub_max * unit + unit // 2
    assert 0 < cap < 2**31 and cap // unit == sub_max             # the switch is read into an int
    return cap


def _borders(sub_max, B):
    """(first - 1, first) for every sub-batch after the first one."""
    return [(first - 1, first) for first in range(sub_max, B, sub_max)]


def _assert_tables_differ_across_a_border(e, sub_max, B):
    """The per-LWE table choices of the batch tell a sub-batch with a wrong offset from a right one: some LWE's table
    differs from its predecessor's across a border, and some LWE beyond the first sub-batch has another table than the
    LWE at the same place of the first sub-batch (what a lut_idx without `+ first` would read)."""
    _, sel, _ = _pairs(e)
    tiled = sel[np.arange(B) % len(sel)]
    assert any(tiled[a] != tiled[b] for a, b in _borders(sub_max, B)), (e.p.name, sub_max, B)
    assert any(tiled[i] != tiled[i % sub_max] for i in range(sub_max, B)), (e.p.name, sub_max, B)


@pytest.mark.parametrize("p,G", SPLIT, ids=_ids(SPLIT))
@pytest.mark.parametrize("sub_max", [3, 5], ids=lambda s: f"sub{s}")
def test_two_kernel_forced_sub_batches(p, G, sub_max, monkeypatch):
    """B = sub_max (one full sub-batch), sub_max + 1 (a second of one LWE), 3 sub_max + 1, 70 (23 or 14 sub-batches, the
    last one partial); the N = 8192 shapes with their rotation workspace behind sub_max prepared LWEs."""
    assert DISTINCT % sub_max != 0
    monkeypatch.setenv(WS_CAP, str(_cap_for(p, G, sub_max)))
    e = _Exact(p, G)
    try:
        for B in (sub_max, sub_max + 1, 3 * sub_max + 1, 70):
            assert min(B, _cap_for(p, G, sub_max) // _per_lwe_bytes(p, G)) == sub_max
            assert len(_borders(sub_max, B)) == (B - 1) // sub_max
            if B == 70:                    # the shuffled choices of one seed may agree at the single border of B = sub_max + 1
                _assert_tables_differ_across_a_border(e, sub_max, B)
            _check(e, B, what=f", sub-batches of {sub_max}")
    finally:
        e.close()


@pytest.mark.parametrize("p,G", [(O.TOY_MULTI_BIT_N256_G3, 3), (O.TOY_MULTI_BIT_N8192, 2)], ids=lambda x: getattr(x, "name", f"G{x}"))
def test_two_kernel_same_batch_whole_and_split(p, G, monkeypatch):
    """The same 70 LWEs on an engine with the automatic cap (one sub-batch) and on one created under the switch (14
    sub-batches of 5): both exact."""
    monkeypatch.delenv(WS_CAP, raising=False)
    _run(p, G, 70)
    monkeypatch.setenv(WS_CAP, str(_cap_for(p, G, 5)))
    e = _Exact(p, G)
    try:
        _assert_tables_differ_across_a_border(e, 5, 70)
        _check(e, 70, what=", sub-batches of 5")
    finally:
        e.close()


@pytest.mark.parametrize("p,G", [(O.TOY_MULTI_BIT_N256, 2), (O.TOY_MULTI_BIT_N8192_G3, 3)], ids=lambda x: getattr(x, "name", f"G{x}"))
def test_two_kernel_workspace_reused_by_a_smaller_batch(p, G):
    """70 LWEs, then 3, then 9 in the workspace the first call left (N = 8192: the rotation workspace moves to behind 3,
    then 9 prepared LWEs inside it), then 70 again."""
    _run(p, G, [70, 3, 9, 70])


# ---- real n ----------------------------------------------------------------------------------------------------------------

REAL_N2048 = [(O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS, 2), (O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS, 3)]


@pytest.mark.parametrize("p,G", REAL_N2048, ids=["N2048_G2_n818", "N2048_G3_n888"])
@pytest.mark.parametrize("combine", [True, False], ids=["combine_prepass", "fused"])
def test_n2048_real_n(p, G, combine):
    """409 and 296 groups: the degree table of lds_per_n * n bytes, key and prepared-GGSW prefetch over hundreds of steps."""
    _run(p, G, 3, setup=None if combine else (lambda eng: eng.set_multibit_combine_max(0)), distinct=3)


def test_two_kernel_real_n():
    """PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3 (N = 512, k = 3, n = 765): 255 groups through the generic combine."""
    _run(O.PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS, 3, 3, distinct=3)
