"""f64 transform precision on every blind-rotation kernel path (tier 2 of tests/test_gpu_exact_rotation.py, path by path).

Tier 1 of that file is bit exact under structured keys, and by construction blind to lost precision: its values sit on the
2^12 grid of from_torus with three orders of magnitude to spare, so twiddles a few bits short pass it.  Its tier 2 measures
precision, on the default path at B = 8 only.  Here the same measurement runs on every path tier 1 reaches, reached the
same way: public setters and batch sizes (choose_rotate_path in csrc/blind_rotate.hip is the map; an MI355X has 256 CUs).

Inputs (exact_pbs.PrecisionCase): a uniformly random full-range key and table and LWEs of one external product each -- one
non-zero mask word (classic) or the n = G twin of the shape (multi-bit) -- so no decomposition digit can differ between two
f64 implementations and the error against the exact integers is the transforms' rounding alone.  Batches above 8 tile 64
distinct LWEs (8 from N = 16384 on), adjacent slots distinct.  The bounds (exact_pbs.assert_f64_precision) are held against the
oracle's f64 spread on at most 16 of the distinct LWEs: pooled spread and maximum, every slot's own spread, no bias.
tests/test_exact_pbs.py shows on the CPU that the oracle's f64 path itself stays inside them.

No rows for throughput mode 2 or keep-busy launches: they run the kernel objects of the B = 257 and B = 8 rows, and a
keyswitch in front cannot produce a one-CMUX input.  profiles/rotation_precision.txt keeps the printed lines of one run."""
import functools

import numpy as np
import pytest

import oracle as O
from exact_pbs import PrecisionCase, assert_f64_precision, signed_errors
from test_gpu_exact_rotation import LARGE, MB_N2048, MB_OTHER, N1024, N2048, _fp, _ksk_len, _shape, _twin

pytestmark = pytest.mark.gpu

DISTINCT = 64


class _Cluster:
    """setup: fhe_engine_set_cluster_mode(mode); a mode other than 0 must have run the multi-CU kernel."""

    def __init__(self, mode):
        self.cluster_mode = mode

    def __call__(self, eng):
        eng.set_cluster_mode(self.cluster_mode)


def _fused(eng):
    eng.set_multibit_combine_max(0)


def _mb(p, G):
    return _twin(p, G, f"{p.name}_n{G}")


SMALL_N = [("N512_K3", _shape("TOY_N512_K3"), 0), ("N512_K2_L2", _shape("TOY_N512_K2_L2"), 0), ("N256_K5", _shape("TOY_N256_K5"), 0),
           ("N256_TOY_K1", O.TOY_K1, 0), ("N256_TOY_K1_wide", O.TOY_K1, 18), ("N128_TOY_K2", O.TOY_K2, 0), ("N128_TOY_K2_wide", O.TOY_K2, 18)]

# (id, shape, G, selector, setup, B)
ROWS = (
    [(f"N2048-variant{s}-B8", N2048, 0, s, None, 8) for s in (2, 3, 4, 18, 19)]
    + [("N2048-two_per_cu-odd_rounds-B257", N2048, 0, 0, None, 257), ("N2048-two_per_cu-even_rounds_fair-B769", N2048, 0, 0, None, 769)]
    + [("N1024-split-B200", N1024, 0, 0, None, 200), ("N1024-variant18_wide_keypf-B200", N1024, 0, 18, None, 200),
       ("N1024-variant2-B8", N1024, 0, 2, None, 8), ("N1024-variant3-B8", N1024, 0, 3, None, 8),
       ("N1024-wide_keypf_variant_large-B300", N1024, 0, 0, None, 300), ("N1024-dense_four_per_cu-B1027", N1024, 0, 0, None, 1027)]
    + [(f"{name}-B515", p, 0, s, None, 515) for name, p, s in SMALL_N]
    + [(f"{p.name}-B515", p, 0, 0, None, 515) for p in (_shape("TOY_N4096_L1"), _shape("TOY_N4096_L2"))]
    + [(f"{p.name}-sequential-B8", p, 0, 0, None, 8) for p in (_shape("TOY_N8192_L1"), O.TOY_N8192)]
    + [(f"{p.name}-cluster{m}-B{B}", p, 0, 0, _Cluster(m), B) for B in (3, 70) for p, m in LARGE]
    + [(f"{p.name}-combine_prepass-B8", _mb(p, G), G, 0, None, 8) for p, G in MB_N2048]
    + [(f"{p.name}-combine_prepass-B64", _mb(p, G), G, 0, None, 64) for p, G in MB_N2048]
    + [(f"{p.name}-fused-B70", _mb(p, G), G, 0, _fused, 70) for p, G in MB_N2048]
    + [(f"{p.name}-two_kernel-B8", _mb(p, G), G, 0, None, 8) for p, G in MB_OTHER]
)


@functools.lru_cache(maxsize=2)                    # rows of one shape follow each other: one reference per (shape, distinct LWEs)
def _case(p, G, D):
    return PrecisionCase(p, G, D)


@pytest.mark.parametrize("name,p,G,selector,setup,B", ROWS, ids=[r[0] for r in ROWS])
def test_rotation_precision(name, p, G, selector, setup, B):
    import fhestr
    D = 8 if B <= 8 or p.N >= 16384 else DISTINCT
    case = _case(p, G, D)
    slots = np.arange(B) % D
    eng = fhestr.Engine(_fp(p, G), 0, selector)
    try:
        eng.load_keys(case.bsk.reshape(-1), np.zeros(_ksk_len(p), dtype=np.uint64))
        if setup:
            setup(eng)
        got = eng.pbs(case.cts[slots], np.full(B, eng.upload_lut(case.lut), dtype=np.uint32))
        if getattr(setup, "cluster_mode", 0):
            assert eng.cluster_info() >= 1         # the multi-CU kernel ran
    finally:
        eng.close()
    assert_f64_precision(name, signed_errors(got, case.want[slots]).reshape(B, -1), case.s_orc, min(B, D))
