"""tests/exact_pbs.py (numpy, exact limb-FFT products) against the C oracle's schoolbook exact path: bit for bit."""
import numpy as np
import pytest

import oracle as O
from conftest import keyset, torus_distance
from exact_pbs import decompose, negacyclic_mul_exact, pbs_exact


def test_negacyclic_limb_product_is_exact():
    rng = np.random.default_rng(1)
    N = 64
    d = rng.integers(-(1 << 14), 1 << 14, size=N)
    key = rng.integers(0, 2**64, size=N, dtype=np.uint64)
    want = np.zeros(N, dtype=object)
    for i in range(N):
        for j in range(N):
            t = int(d[j]) * int(key[(i - j) % N])
            want[i] += -t if j > i else t
    assert [int(v) % 2**64 for v in want] == [int(v) for v in negacyclic_mul_exact(d, key)]


def test_decompose_recomposes():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 2**64, size=1000, dtype=np.uint64)
    for bl, L in ((15, 2), (23, 1), (11, 3), (8, 2)):
        digs = decompose(x, bl, L)
        rec = np.zeros(len(x), dtype=np.uint64)
        with np.errstate(over="ignore"):
            for it, dg in enumerate(digs):                 # it = 0 is level L: weight 2^(64 - bl * L)
                rec += dg.astype(np.uint64) << np.uint64(64 - bl * (L - it))
        err = (rec - x).astype(np.int64)
        assert np.abs(err).max() <= 1 << (63 - bl * L)
        assert all(np.abs(dg).max() <= 1 << (bl - 1) for dg in digs)


@pytest.mark.parametrize("params", [O.TOY_K1, O.TOY_K2, next(p for p in O.TOY_SHAPES if p.name == "TOY_N512_K2_L2")], ids=lambda p: p.name)
def test_numpy_exact_pbs_equals_the_oracles_schoolbook_path(params):
    ks = keyset(params)
    M = params.msg_mod * params.carry_mod
    lut, _ = ks.sk.generate_lookup_table(lambda x: (3 * x + 1) % M)
    cts = ks.ck.encrypt_many([0, 1, M - 1], O.Rng(5, 5))
    for ct in cts:
        small = ks.sk.keyswitch(ct)
        assert np.array_equal(pbs_exact(params, ks.sk.bsk, small, lut), ks.sk.pbs(small, lut, exact=True))
    small = ks.sk.keyswitch(cts[0]).copy()
    small[1] = 0                                           # a_i == 0 is skipped
    assert np.array_equal(pbs_exact(params, ks.sk.bsk, small, lut), ks.sk.pbs(small, lut, exact=True))


# ---- structured keys: a correct f64 PBS is bit exact (the premise of tests/test_gpu_exact_rotation.py) ------------------

from exact_pbs import edge_small_cts, limb_terms, multi_bit_pbs_exact_batch, pbs_exact_batch, structured_bsk   # noqa: E402

N2048_TWIN = O.Params(24, 1, 2048, 23, 1, 3, 5, 4, 4, 1e-13, 1e-17, "TOY_N2048_K1")    # PARAM_MESSAGE_2_CARRY_2's shape, small n
STRUCTURED_SHAPES = [O.TOY_K1, O.TOY_K2, N2048_TWIN] + O.TOY_SHAPES
MULTI_BIT_TOYS = [(O.TOY_MULTI_BIT_N256, 2), (O.TOY_MULTI_BIT_N256_G3, 3), (O.TOY_MULTI_BIT_N128_K2, 2),
                  (O.TOY_MULTI_BIT_N512_K3_G3, 3)]
# the real n of tests/test_gpu_exact_multibit.py: hundreds of groups, each one more rounding of the whole accumulator
MULTI_BIT_REAL_N = [(O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS, 2), (O.PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS, 3),
                    (O.PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS, 3)]


@pytest.mark.parametrize("params", STRUCTURED_SHAPES, ids=lambda p: p.name)
def test_oracle_f64_pbs_is_bit_exact_under_structured_keys(params):
    rng = np.random.default_rng(params.N * 31 + params.k)
    bsk, terms, _ = structured_bsk(params, rng)
    ksk = np.zeros(params.big_dim * params.ks_level * params.small_size, dtype=np.uint64)
    sk = O.ServerKey.from_keys(params, bsk, ksk, threads=1)
    luts = rng.integers(0, 2**64, size=(2, params.glwe_len), dtype=np.uint64)
    cts = edge_small_cts(params, rng, 3)
    idx = np.array([0, 1, 0])
    want = pbs_exact_batch(params, terms, cts, luts, idx)
    got = np.stack([sk.pbs(c, luts[i]) for c, i in zip(cts, idx)])
    _assert_on_grid(got, want, params)


def _assert_on_grid(got, want, params):
    """The oracle's f64 path (the reference's from_torus) rounds every product to the 2^-64 grid, so its own transform
    error -- a few units there, summed over the n steps -- shows in the output.  The engine rounds to the 2^-52 grid, on
    which every product of a structured key lies (t >= 12): a correct f64 PBS is then bit exact as long as that error
    stays far below half a grid step, 2^11.  Asserted with a 2^5 margin (measured: at most a few units; 0 below N = 2048)."""
    dist = torus_distance(got, want)
    print(f"{params.name}: {int((dist > 0).sum())} of {dist.size} coefficients off the exact value, max {int(dist.max())} (2^-64 units)")
    assert dist.max() < 2.0**6


def test_structured_key_premise_fails_with_wide_coefficients():
    """Negative control: 20-bit c breaks the f64 exactness the structured keys rely on."""
    params = next(p for p in O.TOY_SHAPES if p.name == "TOY_N1024_K2")
    rng = np.random.default_rng(3)
    bsk, (c_t,), t = structured_bsk(params, rng)
    c = rng.integers(-(1 << 19), 1 << 19, size=c_t[0].shape, dtype=np.int64)
    bsk = c.astype(np.uint64) << np.uint64(t)
    ksk = np.zeros(params.big_dim * params.ks_level * params.small_size, dtype=np.uint64)
    sk = O.ServerKey.from_keys(params, bsk, ksk, threads=1)
    lut = rng.integers(0, 2**64, size=params.glwe_len, dtype=np.uint64)
    cts = edge_small_cts(params, rng, 1)
    assert torus_distance(sk.pbs(cts[0], lut), pbs_exact_batch(params, limb_terms(bsk), cts, lut)[0]).max() > 2.0**11


@pytest.mark.parametrize("params", [O.TOY_K1, O.TOY_K2, next(p for p in O.TOY_SHAPES if p.name == "TOY_N512_K2_L2")], ids=lambda p: p.name)
def test_batched_exact_pbs_equals_the_oracles_schoolbook_path(params):
    """pbs_exact_batch on full-range keys (eight limb terms) against orc_pbs_exact, per-LWE tables."""
    ks = keyset(params)
    rng = np.random.default_rng(9)
    luts = rng.integers(0, 2**64, size=(2, params.glwe_len), dtype=np.uint64)
    cts = edge_small_cts(params, rng, 3)
    idx = np.array([1, 0, 1])
    want = np.stack([ks.sk.pbs(c, luts[i], exact=True) for c, i in zip(cts, idx)])
    assert np.array_equal(pbs_exact_batch(params, limb_terms(ks.sk.bsk.reshape(params.n, params.pbs_level, params.k + 1, params.k + 1, params.N)), cts, luts, idx), want)


@pytest.mark.parametrize("params,G", MULTI_BIT_TOYS, ids=lambda x: getattr(x, "name", f"G{x}"))
def test_numpy_multi_bit_pbs_equals_the_oracles_exact_path(params, G):
    ck = O.ClientKey(params, 0x4D420001)
    sk = O.MultiBitServerKey(ck, G, threads=1)
    rng = np.random.default_rng(G * 100 + params.N)
    luts = rng.integers(0, 2**64, size=(2, params.glwe_len), dtype=np.uint64)
    cts = edge_small_cts(params, rng, 2)
    idx = np.array([0, 1])
    want = np.stack([sk.pbs(c, luts[i], exact=True) for c, i in zip(cts, idx)])
    shape = (sk.n_ggsw, params.pbs_level, params.k + 1, params.k + 1, params.N)
    assert np.array_equal(multi_bit_pbs_exact_batch(params, G, limb_terms(sk.bsk.reshape(shape)), cts, luts, idx), want)


@pytest.mark.parametrize("params,G", MULTI_BIT_TOYS + [(O.TOY_MULTI_BIT_N2048_G3, 3), (O.TOY_MULTI_BIT_N8192, 2)] + MULTI_BIT_REAL_N,
                         ids=lambda x: getattr(x, "name", f"G{x}"))
def test_oracle_f64_multi_bit_pbs_is_bit_exact_under_structured_keys(params, G):
    rng = np.random.default_rng(G * 1000 + params.N)
    bsk, terms, _ = structured_bsk(params, rng, grouping=G)
    sk = O.MultiBitServerKey.from_keys(params, G, bsk, threads=1)
    luts = rng.integers(0, 2**64, size=(2, params.glwe_len), dtype=np.uint64)
    cts = edge_small_cts(params, rng, 2)
    idx = np.array([1, 0])
    want = multi_bit_pbs_exact_batch(params, G, terms, cts, luts, idx)
    got = np.stack([sk.pbs(c, luts[i]) for c, i in zip(cts, idx)])
    _assert_on_grid(got, want, params)


# ---- full-range keys: the oracle's f64 path stays inside the precision bounds (the premise of tests/test_gpu_rotation_precision.py) ---

from exact_pbs import ORACLE_ROWS, PrecisionCase, assert_f64_precision, f64_precision_figures, twin   # noqa: E402

PRECISION_SHAPES = [twin(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 8, "TOY_N2048_K1"), twin(O.PARAM_MESSAGE_2_CARRY_1_KS_PBS, 8, "TOY_N1024_K2_n8"),
                    O.TOY_K2, next(p for p in O.TOY_SHAPES if p.name == "TOY_N4096_L2")]


@pytest.mark.parametrize("params", PRECISION_SHAPES, ids=lambda p: p.name)
def test_oracle_f64_pbs_meets_the_precision_bounds(params):
    """The three bounds of assert_f64_precision with the oracle's f64 output in the GPU's place: 16 one-CMUX LWEs under one
    full-range key, held against the oracle's spread on 16 others under another key (a second seed).  A correct f64
    implementation reaches the bounds, and every coefficient carries an error: none of the measurement is vacuous."""
    ref, other = PrecisionCase(params, 0, ORACLE_ROWS, seed=0), PrecisionCase(params, 0, ORACLE_ROWS, seed=1)
    assert (other.e_orc != 0).mean() > 0.99
    f = assert_f64_precision(params.name, other.e_orc, ref.s_orc, ORACLE_ROWS)
    assert 0.8 < f["ratio"] < 1.25                     # the spread varies a little from LWE to LWE (digits, table); 16 of them pooled agree well within a quarter


def test_precision_bounds_catch_a_lost_bit_a_truncation_and_one_bad_slot():
    """Negative controls on the oracle's own error: twice the spread, an offset of half a sigma, one slot of 16 at 2.5 times the noise."""
    case = PrecisionCase(O.TOY_K2, 0, ORACLE_ROWS)
    e, s = case.e_orc, case.s_orc
    f64_precision_figures(e, s, ORACLE_ROWS)
    with pytest.raises(AssertionError):
        assert_f64_precision("doubled", 2 * e, s, ORACLE_ROWS)
    with pytest.raises(AssertionError):
        assert_f64_precision("offset", e - 0.5 * s, s, ORACLE_ROWS)
    one = e.copy()
    one[5] *= 2.5
    assert one.std() <= 1.6 * s                       # diluted in the pool: only the per-slot bound sees it
    with pytest.raises(AssertionError):
        assert_f64_precision("one slot", one, s, ORACLE_ROWS)
