"""Every blind-rotation kernel path against exact integers (tests/exact_pbs.py).

Tier 1, bit exact: under a structured bootstrapping key (every word c << t, |c| < 2^7, t >= 12: exact_pbs.structured_bsk)
every value of a correct f64 PBS lies on the engine's from_torus grid with a wide margin (tests/test_exact_pbs.py pins
that premise on the CPU oracle), so the whole output ciphertext -- mask and body -- must equal the exact integer PBS bit
for bit.  A transform that lost precision, a wrong twiddle, a swapped GGSW block, level or sign shows as a mismatch.
Each path is reached through the public setters and batch sizes only (choose_rotate_path in csrc/blind_rotate.hip is
the map; an MI355X has 256 CUs).  Multi-bit here runs B = 5 on every shape; its batch regimes -- the combined prepass's chunks
of 8 up to multibit_combine_max = 64, the fused kernel from 65 on and beyond the CU count, the two-kernel path's sub-batch
loop (reached through the environment switch FHESTR_MULTIBIT_WS_CAP, bytes, read when an engine is created) and real n --
are in tests/test_gpu_exact_multibit.py, on this file's rig.

Tier 2, full scale: uniformly random keys and LWEs with exactly one non-zero mask element (one CMUX, no decomposition
digit can differ): the engine's per-coefficient error against exact must have the spread of the oracle's f64 path.  Here on the
default path at B = 8; path by path, where tier 1's grid margin hides a loss of up to a dozen bits, in tests/test_gpu_rotation_precision.py."""
import numpy as np
import pytest

import oracle as O
from conftest import torus_distance
from exact_keyswitch import ExactKeyswitch, edge_big_cts
from exact_pbs import (edge_small_cts, limb_terms, multi_bit_pbs_exact_batch, pbs_exact_batch, structured_bsk)
from exact_pbs import one_cmux_inputs as _one_cmux_inputs, signed_errors as _errors, twin as _twin      # shared with the CPU tests

pytestmark = pytest.mark.gpu

DISTINCT = 64            # large batches tile this many distinct (ciphertext, table) pairs, adjacent slots distinct
N_LUTS = 3


def _shape(name):
    return next(p for p in O.TOY_SHAPES if p.name == name)


P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
P21 = O.PARAM_MESSAGE_2_CARRY_1_KS_PBS
N2048 = _twin(P22, 8, "TOY_N2048_K1")
N1024 = _twin(P21, 8, "TOY_N1024_K2_n8")


def _fp(p, G=0):
    import fhestr
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name, G or 1)


def _ksk_len(p):
    return p.k * p.N * p.ks_level * (p.n + 1)


class _Exact:
    """A fresh engine holding a structured key (closed by close()), random full-range tables and the exact reference."""

    def __init__(self, p, G=0, selector=0, seed=0):
        import fhestr
        self.p, self.G = p, G
        self.rng = np.random.default_rng([p.N, p.k, p.pbs_level, p.n, G, selector, seed])
        bsk, self.terms, _ = structured_bsk(p, self.rng, grouping=G)
        self.ksk = self.rng.integers(0, 2**64, size=_ksk_len(p), dtype=np.uint64)
        self.eng = fhestr.Engine(_fp(p, G), 0, selector)
        self.eng.load_keys(bsk.reshape(-1), self.ksk)
        self.bsk = bsk
        self.luts = self.rng.integers(0, 2**64, size=(N_LUTS, p.glwe_len), dtype=np.uint64)
        self.ids = np.array([self.eng.upload_lut(lut) for lut in self.luts], dtype=np.uint32)

    def reference(self, cts, sel):
        if self.G:
            return multi_bit_pbs_exact_batch(self.p, self.G, self.terms, cts, self.luts, sel)
        return pbs_exact_batch(self.p, self.terms, cts, self.luts, sel)

    def inputs(self, B):
        """B small-key LWEs (tiled from at most DISTINCT distinct ones), per-LWE table choices, exact outputs per slot."""
        D = min(B, DISTINCT)
        cts = edge_small_cts(self.p, self.rng, D)
        sel = np.arange(D) % N_LUTS
        self.rng.shuffle(sel)
        want = self.reference(cts, sel)
        slots = np.arange(B) % D
        return cts[slots], sel[slots], want[slots]

    def check(self, B):
        cts, sel, want = self.inputs(B)
        got = self.eng.pbs(cts, self.ids[sel])
        _assert_exact(got, want)

    def close(self):
        self.eng.close()


def _assert_exact(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        d = torus_distance(got, want)
        raise AssertionError(f"{len(bad)} of {len(want)} LWEs differ from exact (first {bad[:8].tolist()}): "
                             f"{int((d > 0).sum())} coefficients, max distance 2^{np.log2(d.max()):.1f}")


def _run(p, B, G=0, selector=0, setup=None):
    e = _Exact(p, G, selector)
    try:
        if setup:
            setup(e.eng)
        e.check(B)
    finally:
        e.close()


# ---- tier 1: N = 2048, k = 1, L = 1 (PARAM_MESSAGE_2_CARRY_2's shape) ---------------------------------------------------

@pytest.mark.parametrize("selector", [2, 3, 4, 18, 19], ids=lambda s: f"variant{s}")
def test_n2048_variant(selector):
    _run(N2048, 5, selector=selector)


@pytest.mark.parametrize("B", [1, 3, 256, 257, 515, 769], ids=lambda b: f"B{b}")
def test_n2048_default_dispatch(B):
    """<= 256: one LWE per CU; above: the two-LWEs-per-CU kernel, time-sliced priorities on for an even number of rounds."""
    _run(N2048, B)


def test_n2048_keep_busy_B3():
    _run(N2048, 3, setup=lambda eng: eng.set_keep_busy(True))


def test_n2048_real_n():
    _run(P22, 4)


def _pipeline_mode2(p, B=96, calls=3):
    """fhe_engine_set_pipeline(2): consecutive apply_lookup_table_dev calls overlapped on two streams.  The keyswitch
    is the exact-integer one of tests/exact_keyswitch.py, on all-distinct edge rows; each call's output against the exact
    PBS of that, bit for bit."""
    import torch
    e = _Exact(p)
    try:
        keyswitch = ExactKeyswitch(p, e.ksk)
        big = [edge_big_cts(p, e.rng, B) for _ in range(calls)]
        sel = [np.arange(B) % N_LUTS for _ in range(calls)]
        wants = [e.reference(keyswitch(b), s) for b, s in zip(big, sel)]
        ins = [torch.from_numpy(b.view(np.int64)).cuda() for b in big]
        idx = [torch.from_numpy(e.ids[s].astype(np.int32)).cuda() for s in sel]
        outs = [torch.zeros_like(t) for t in ins]
        torch.cuda.synchronize()                   # torch's stream is not ordered with the engine's
        e.eng.set_pipeline(2)
        try:
            for i, o, x in zip(ins, outs, idx):
                e.eng.apply_lookup_table_dev(i.data_ptr(), x.data_ptr(), o.data_ptr(), B)
            e.eng.synchronize()
        finally:
            e.eng.set_pipeline(0)
        for o, want in zip(outs, wants):
            _assert_exact(o.cpu().numpy().view(np.uint64), want)
    finally:
        e.close()


def test_n2048_pipeline_mode2():
    _pipeline_mode2(N2048)


# ---- N = 1024, k = 2 ----------------------------------------------------------------------------------------------------

def test_n1024_split_kernel():
    _run(N1024, 200)


def test_n1024_wide_kernel_key_prefetch():
    _run(N1024, 200, selector=18)


def test_n1024_dense_four_per_cu():
    _run(N1024, 1027)


def test_n1024_pipeline_mode2():
    _pipeline_mode2(N1024)


@pytest.mark.parametrize("selector", [2, 3, 18], ids=lambda s: f"variant{s}")
def test_n1024_variant(selector):
    _run(N1024, 5, selector=selector)


def test_n1024_real_n():
    _run(P21, 3)


# ---- small N: 512, 256, 128 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,selector", [(_shape("TOY_N512_K3"), 0), (_shape("TOY_N512_K2_L2"), 0), (_shape("TOY_N256_K5"), 0),
                                        (O.TOY_K1, 0), (O.TOY_K1, 18), (O.TOY_K2, 0), (O.TOY_K2, 18)],
                         ids=["N512_K3", "N512_K2_L2", "N256_K5", "N256_TOY_K1", "N256_TOY_K1_wide", "N128_TOY_K2", "N128_TOY_K2_wide"])
@pytest.mark.parametrize("B", [5, 515], ids=lambda b: f"B{b}")
def test_small_n(p, selector, B):
    _run(p, B, selector=selector)


# ---- N = 4096 and 8192 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [_shape("TOY_N4096_L1"), _shape("TOY_N4096_L2")], ids=lambda p: p.name)
@pytest.mark.parametrize("B", [3, 515], ids=lambda b: f"B{b}")
def test_n4096(p, B):
    _run(p, B)


@pytest.mark.parametrize("p", [_shape("TOY_N8192_L1"), O.TOY_N8192], ids=lambda p: p.name)
def test_n8192_sequential_kernel(p):
    _run(p, 5)


# ---- N = 16384 and 32768: one workgroup per LWE (mode 0), clusters of CUs (1), the whole-XCD kernel (N = 32768, L = 2) -

LARGE = [(_shape("TOY_N16384_L2"), 0), (_shape("TOY_N16384_L2"), 1), (_shape("TOY_N16384_L3"), 0), (_shape("TOY_N16384_L3"), 1),
         (O.TOY_N32768, 0), (O.TOY_N32768, 1), (O.TOY_N32768, 2), (_shape("TOY_N32768_L3"), 0), (_shape("TOY_N32768_L3"), 1)]


@pytest.mark.parametrize("p,mode", LARGE, ids=[f"{p.name}-cluster{m}" for p, m in LARGE])
@pytest.mark.parametrize("B", [3, 70], ids=lambda b: f"B{b}")
def test_large_n(p, mode, B):
    """B = 3: the whole-XCD kernel in mode 1 on N = 32768, L = 2; B = 70: more LWEs than any launch forms clusters."""
    e = _Exact(p)
    try:
        e.eng.set_cluster_mode(mode)
        e.check(B)
        if mode:
            assert e.eng.cluster_info() >= 1          # the multi-CU kernel ran
    finally:
        e.close()


# ---- multi-bit -----------------------------------------------------------------------------------------------------------

MB_N2048 = [(O.TOY_MULTI_BIT_N2048, 2), (O.TOY_MULTI_BIT_N2048_G3, 3)]
MB_OTHER = [(_twin(O.TOY_MULTI_BIT_N512_K3_G3, 8, "TOY_MULTI_BIT_N512_K3_G2"), 2), (O.TOY_MULTI_BIT_N512_K3_G3, 3),
            (O.TOY_MULTI_BIT_N8192, 2), (O.TOY_MULTI_BIT_N8192_G3, 3),
            (O.TOY_MULTI_BIT_N256, 2), (O.TOY_MULTI_BIT_N256_G3, 3),
            (O.TOY_MULTI_BIT_N128_K2, 2), (_twin(O.TOY_MULTI_BIT_N128_K2, 12, "TOY_MULTI_BIT_N128_K2_G3"), 3)]


@pytest.mark.parametrize("p,G", MB_N2048, ids=[p.name for p, _ in MB_N2048])
@pytest.mark.parametrize("combine", [True, False], ids=["combine_prepass", "fused"])
def test_multi_bit_n2048(p, G, combine):
    _run(p, 5, G=G, setup=None if combine else (lambda eng: eng.set_multibit_combine_max(0)))


@pytest.mark.parametrize("p,G", MB_OTHER, ids=[p.name for p, _ in MB_OTHER])
def test_multi_bit_two_kernel_path(p, G):
    _run(p, 5, G=G)


# ---- tier 2: transform precision at full scale ---------------------------------------------------------------------------

FULL = [N2048, N1024, _shape("TOY_N512_K3"), _shape("TOY_N256_K5"), O.TOY_K2, _shape("TOY_N4096_L2"), O.TOY_N8192,
        _shape("TOY_N16384_L3"), O.TOY_N32768]
FULL_MB = [(_twin(O.TOY_MULTI_BIT_N2048, 2, "TOY_MULTI_BIT_N2048_G2_n2"), 2),
           (_twin(O.TOY_MULTI_BIT_N8192_G3, 3, "TOY_MULTI_BIT_N8192_G3_n3"), 3)]


def _precision(name, eng_out, orc_out, want):
    e_gpu, e_orc = _errors(eng_out, want), _errors(orc_out, want)
    s_gpu, s_orc = e_gpu.std(), e_orc.std()
    print(f"{name}: error std GPU 2^{np.log2(s_gpu):.2f}, oracle f64 2^{np.log2(s_orc):.2f} (ratio {s_gpu / s_orc:.3f}); "
          f"GPU max 2^{np.log2(np.abs(e_gpu).max()):.2f}")
    assert 0.25 * s_orc < s_gpu <= 1.6 * s_orc
    assert np.abs(e_gpu).max() < 8 * s_orc


@pytest.mark.parametrize("p", FULL, ids=lambda p: p.name)
def test_full_scale_precision(p):
    import fhestr
    rng = np.random.default_rng([p.N, p.k, p.pbs_level, 2])
    bsk = rng.integers(0, 2**64, size=(p.n, p.pbs_level, p.k + 1, p.k + 1, p.N), dtype=np.uint64)
    sk = O.ServerKey.from_keys(p, bsk, np.zeros(_ksk_len(p), dtype=np.uint64), threads=4)
    lut = rng.integers(0, 2**64, size=p.glwe_len, dtype=np.uint64)
    B = 8
    cts = _one_cmux_inputs(p, rng, B)
    want = pbs_exact_batch(p, limb_terms(bsk), cts, lut)
    orc = np.stack([sk.pbs(c, lut) for c in cts])
    eng = fhestr.Engine(_fp(p), 0)
    try:
        eng.load_keys(bsk.reshape(-1), np.zeros(_ksk_len(p), dtype=np.uint64))
        got = eng.pbs(cts, np.full(B, eng.upload_lut(lut), dtype=np.uint32))
    finally:
        eng.close()
    _precision(p.name, got, orc, want)


@pytest.mark.parametrize("p,G", FULL_MB, ids=[p.name for p, _ in FULL_MB])
def test_full_scale_precision_multi_bit(p, G):
    """n = G: a single group, so one external product of the combined GGSW with the rotated table."""
    import fhestr
    rng = np.random.default_rng([p.N, G, 3])
    n_ggsw = p.n // G * (1 << G)
    bsk = rng.integers(0, 2**64, size=(n_ggsw, p.pbs_level, p.k + 1, p.k + 1, p.N), dtype=np.uint64)
    sk = O.MultiBitServerKey.from_keys(p, G, bsk, threads=4)
    lut = rng.integers(0, 2**64, size=p.glwe_len, dtype=np.uint64)
    B = 8
    cts = rng.integers(0, 2**64, size=(B, p.n + 1), dtype=np.uint64)
    want = multi_bit_pbs_exact_batch(p, G, limb_terms(bsk), cts, lut)
    orc = np.stack([sk.pbs(c, lut) for c in cts])
    eng = fhestr.Engine(_fp(p, G), 0)
    try:
        eng.load_keys(bsk.reshape(-1), np.zeros(_ksk_len(p), dtype=np.uint64))
        got = eng.pbs(cts, np.full(B, eng.upload_lut(lut), dtype=np.uint32))
    finally:
        eng.close()
    _precision(p.name, got, orc, want)
