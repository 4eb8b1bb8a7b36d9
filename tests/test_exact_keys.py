"""The noise sampler (csrc/det_math.h) against a real logarithm and a real normal distribution, and the host client's server
keys against the definition of an LWE / GLWE / GGSW encryption (tests/exact_keys.py).  Host, device and oracle share the
sampler's formulas, so their word-for-word agreement says nothing about a wrong coefficient, a dropped factor or a
repeated stream; these tests do.  tests/test_gpu_exact_keys.py repeats the key checks on device-generated keys."""
import math

import numpy as np
import pytest

import oracle as O
import exact_keys as X
import key_cases as K

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
SMALLEST_TOY_GLWE_STD = min(p.glwe_std for p in [O.TOY_K1, O.TOY_K2, O.TOY_N8192, O.TOY_N32768] + O.TOY_SHAPES)   # 1e-17: sigma = 184

# largest det_log error measured on the inputs below, in ulp of the true value (x86-64, 80-bit longdouble reference)
DET_LOG_MEASURED_ULP = 1.86


def _det_log_inputs():
    rng = np.random.default_rng(0xD37)
    xs = [np.exp2(rng.uniform(-126.0, 0.0, 1_000_000))]                    # log-uniform over [2^-126, 1)
    edges = np.exp2(np.arange(-126, 1).astype(np.float64))                  # every binade edge and its two neighbours
    xs += [edges, np.nextafter(edges, 0.0), np.nextafter(edges, 2.0)]
    for e in (-126, -100, -64, -31, -10, -2, -1):                           # the reduction boundary m = sqrt 2, +- 4 ulp
        b = np.float64(math.sqrt(2.0)) * 2.0 ** e
        lo, hi = [b], [b]
        for _ in range(4):
            lo.append(np.nextafter(lo[-1], 0.0))
            hi.append(np.nextafter(hi[-1], 4.0))
        xs.append(np.array(lo + hi))
    xs.append(1.0 - 2.0 ** -53 * np.arange(1, 65))                          # just below 1
    x = np.concatenate(xs)
    return x[(x > 0.0) & (x < 1.0)]


def test_det_log_against_a_real_logarithm():
    """det_log on what the polar method can hand it -- s = u^2 + v^2 strictly inside (0, 1), u and v multiples of 2^-63, so
    down to 2^-126 -- against numpy.log in longdouble (64-bit mantissa here, 11 bits more than f64).  Largest error
    measured: 1.86 ulp of the true value, at x = 0.6916 where e ln 2 and the series cancel (mean 0.25 ulp); the bound is four
    times that, 7.44 ulp.  Where longdouble is no wider than double the reference is math.log and the margin eight times."""
    import fhestr
    x = _det_log_inputs()
    got = fhestr.debug_det_log(x)
    if np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant:
        ref, margin = np.log(x.astype(np.longdouble)), 4.0
    else:
        ref, margin = np.array([math.log(v) for v in x], dtype=np.longdouble), 8.0
    ulp = np.spacing(np.abs(ref.astype(np.float64)))
    err = np.abs(got.astype(np.longdouble) - ref) / ulp
    worst = int(err.argmax())
    print(f"det_log: max error {float(err.max()):.3f} ulp at x = {x[worst]!r}, mean {float(err.mean()):.3f} ulp, {x.size} inputs")
    assert float(err.max()) <= margin * DET_LOG_MEASURED_ULP, (float(err.max()), x[worst])


def test_round_half_away_and_from_torus_exact_at_their_edges():
    import fhestr
    two52 = 2.0 ** 52
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.0, -0.0, 0.49999999999999994, -0.49999999999999994, 0.75, -0.75,
                  two52, -two52, two52 - 0.5, -(two52 - 0.5), two52 - 1.0, two52 + 2.0, 2.0 ** 62, -1e300])
    want = np.array([1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.0, 0.0, 0.0, 0.0, 1.0, -1.0,
                     two52, -two52, two52, -two52, two52 - 1.0, two52 + 2.0, 2.0 ** 62, -1e300])
    rounded, _ = fhestr.debug_round_torus(x)
    assert np.array_equal(rounded, want)
    # from_torus_exact: the fractional part of x times 2^64, ties away from zero, saturating where it reaches +-2^63
    below_half = float(np.nextafter(0.5, 0.0))                  # 0.5 - 2^-54 -> 2^63 - 2^10
    cases = [(0.0, 0), (0.25, 1 << 62), (-0.25, -(1 << 62)), (1.25, 1 << 62), (-3.25, -(1 << 62)),
             (0.5, -(1 << 63)),                                 # 0.5 - round(0.5) = -0.5: saturates at INT64_MIN
             (-0.5, (1 << 63) - 1),                             # -0.5 + 1 = 0.5 -> 2^63: saturates at INT64_MAX
             (below_half, (1 << 63) - (1 << 10)), (-below_half, -(1 << 63) + (1 << 10)),
             (2.0 ** -64, 1), (-2.0 ** -64, -1), (2.0 ** -65, 1), (-2.0 ** -65, -1), (2.0 ** -66, 0), (3 * 2.0 ** -65, 2)]
    _, torus = fhestr.debug_round_torus(np.array([c[0] for c in cases]))
    assert torus.view(np.int64).tolist() == [c[1] for c in cases]


def _polar_reference(seed, stream, std, count):
    """gaussian.rs:17-47 restated on the raw ChaCha20 words: pairs of signed 64-bit draws scaled to [-1, 1), rejected unless
    0 < s = u^2 + v^2 < 1, FIRST sample u sqrt(-2 ln s / s) times std, as a torus integer; longdouble and a real log."""
    import fhestr
    ld = np.longdouble
    words, block, out = [], 0, []
    while len(out) < count:
        while len(words) < 2:
            b = fhestr.chacha20_block(seed, block, stream).astype(np.uint64)
            words += [int(b[2 * i]) | (int(b[2 * i + 1]) << 32) for i in range(8)]
            block += 1
        u, v = (ld(w - (1 << 64) if w >> 63 else w) / ld(2.0 ** 63) for w in (words.pop(0), words.pop(0)))
        s = u * u + v * v
        if 0 < s < 1:
            out.append(u * ld(std) * np.sqrt(ld(-2.0) * np.log(s) / s) * ld(2.0 ** 64))
    return np.array(out, dtype=ld)


@pytest.mark.parametrize("std", [P22.lwe_std, P22.glwe_std], ids=["p22_lwe_std", "p22_glwe_std"])
def test_samples_are_the_first_of_the_polar_pair_with_a_real_logarithm(std):
    """Sample by sample: the sampler's values equal the polar method's first sample computed with numpy's logarithm in
    longdouble from the same stream, to within its own f64 roundings (some twenty operations and det_log's 7.4 ulp: 64 ulp
    of the value is generous and still 1e8 times below a wrong coefficient or the other sample of the pair) plus one for
    the final rounding to an integer."""
    import fhestr
    seed, stream, count = 0x5A17, 0x99, 1500
    got = fhestr.debug_noise_samples(seed, stream, std, count).view(np.int64)
    want = _polar_reference(seed, stream, std, count)
    err = np.abs(got.astype(np.longdouble) - want)
    assert (err <= 1.0 + 64 * 2.0 ** -53 * np.abs(want)).all(), float(err.max())


@pytest.mark.parametrize("stream, std", [(7, P22.lwe_std), (17, P22.glwe_std), (27, SMALLEST_TOY_GLWE_STD)],
                         ids=["p22_lwe_std", "p22_glwe_std", "toy_glwe_std"])
def test_sampler_distribution(stream, std):
    """4e6 consecutive draws of one stream at three deviations through normal_checks; a stream is reproducible, two streams
    differ and share no more values than honest samples do; consecutive draws are uncorrelated."""
    import fhestr
    M = 4_000_000
    e = fhestr.debug_noise_samples(0x5A17, stream, std, M).view(np.int64)
    print(f"std {std:g}: var/sigma^2 = {X.variance_ratio(e, std):.5f}")
    X.normal_checks(e, std, f"sampler at std {std:g}")
    again = fhestr.debug_noise_samples(0x5A17, stream, std, 4096).view(np.int64)
    other = fhestr.debug_noise_samples(0x5A17, stream + 1, std, 4096).view(np.int64)
    assert np.array_equal(again, e[:4096]) and not np.array_equal(other, e[:4096])
    assert X._equal_pairs(np.concatenate([other, e[:4096]])) <= X.repeat_bound(8192, std * 2.0 ** 64)[1]
    x = e.astype(np.float64)
    x -= x.mean()
    lag1 = float((x[:-1] * x[1:]).mean() / (x * x).mean())
    assert abs(lag1) <= 6.0 / math.sqrt(M), lag1          # independent draws: the lag-1 autocorrelation has deviation 1 / sqrt M


def test_every_seed_word_reaches_the_streams():
    """Seeds that differ in one of the eight 32-bit words of the ChaCha20 key give different noise and different keys.
    seed_bytes carries all eight: an int is laid out little endian over the 32 bytes (tests mostly pass ints below 2^32,
    word 0 only), so word w is reached with 1 << 32 w; there is no word it cannot reach."""
    import fhestr
    base = 0x0123456789ABCDEF_0F1E2D3C4B5A6978_1122334455667788_99AABBCCDDEEFF00
    seeds = [base] + [base ^ (1 << (32 * w)) for w in range(8)]
    assert [fhestr.seed_bytes(s) for s in seeds[1:]] == [bytes(b ^ (1 if i == 4 * w else 0) for i, b in enumerate(fhestr.seed_bytes(base)))
                                                          for w in range(8)]
    noise = [fhestr.debug_noise_samples(s, 1, 1e-15, 64).tobytes() for s in seeds]
    assert len(set(noise)) == 9
    case = K.BY_NAME[O.TOY_K2.name]
    keys = []
    for s in seeds:
        ck = fhestr.ClientKey(K.fhestr_params(case), s)
        bsk, ksk = ck.gen_server_keys(2)
        keys.append((ck.secret_keys()[0].tobytes(), bsk.tobytes(), ksk.tobytes()))
    for part in range(3):
        assert len({k[part] for k in keys}) == 9


def test_ggsw_bits_select_exactly_one_monomial():
    """The multi-bit PBS multiplies the accumulator by sum_sel GGSW_sel X^(sum of a_b over the b whose selector bit G-1-b is
    set) (lwe_multi_bit_programmable_bootstrapping.rs:53-62); with the plaintext bits of ggsw_bits that sum has to be the one
    monomial X^(sum_b s_b a_b), for every key pattern -- so for every selector -- and exponents that tell all subsets apart."""
    for G in (2, 3):
        a = [3 ** b for b in range(G)]                      # distinct subset sums
        p = O.Params(G, 1, 128, 10, 1, 3, 3, 2, 2, 1e-12, 1e-15, "group")
        seen = set()
        for pattern in range(1 << G):
            s = np.array([(pattern >> b) & 1 for b in range(G)], dtype=np.uint64)
            bits = X.ggsw_bits(p, s, G)
            poly = np.zeros(2 * p.N, dtype=np.int64)
            for sel in range(1 << G):
                poly[sum(a[b] for b in range(G) if (sel >> (G - 1 - b)) & 1)] += int(bits[sel])
            want = np.zeros(2 * p.N, dtype=np.int64)
            want[sum(int(s[b]) * a[b] for b in range(G))] = 1
            assert np.array_equal(poly, want), (G, pattern)
            seen.add(int(np.flatnonzero(bits)[0]))
        assert seen == set(range(1 << G))


def test_the_checks_tell_right_from_wrong():
    """normal_checks passes numpy's own normal samples and fails on a variance 2 % off, a mean 0.5 % of sigma off and a
    lost tail; it raises below sigma = 2^6; distinct_streams sees one repeated row."""
    rng = np.random.default_rng(5)
    std, M = 1e-15, 200_000
    sigma = std * 2.0 ** 64
    good = np.rint(rng.normal(0.0, sigma, M)).astype(np.int64)
    X.normal_checks(good, std, "numpy")
    for bad in (np.rint(good * 1.02).astype(np.int64), good + int(0.02 * sigma), np.clip(good, -2.5 * sigma, 2.5 * sigma).astype(np.int64),
                np.rint(good / math.sqrt(2.0)).astype(np.int64)):
        with pytest.raises(AssertionError):
            X.normal_checks(bad, std, "bad")
    with pytest.raises(ValueError):
        X.normal_checks(good, 63.0 / 2.0 ** 64, "tiny")
    p = O.TOY_K2
    ksk = rng.integers(0, 1 << 63, size=p.big_dim * p.ks_level * (p.n + 1), dtype=np.uint64)
    bsk = rng.integers(0, 1 << 63, size=p.n * p.pbs_level * (p.k + 1) ** 2 * p.N, dtype=np.uint64)
    X.distinct_streams(ksk, bsk, p)
    bsk[5 * (p.k + 1) * p.N] = ksk[7 * (p.n + 1)]
    with pytest.raises(AssertionError):
        X.distinct_streams(ksk, bsk, p)
    with pytest.raises(AssertionError):
        X.distinct_streams(ksk, rng.integers(0, 1 << 63, size=bsk.size, dtype=np.uint64), p, ksk_res=np.tile(good[:500], 2))


def test_negacyclic_product_against_the_schoolbook():
    rng = np.random.default_rng(6)
    A = rng.integers(0, 1 << 63, size=(3, 64), dtype=np.uint64) * np.uint64(3)
    S = rng.integers(0, 2, size=64, dtype=np.uint64)
    S[[0, 63]] = 1
    got = X.negacyclic_by_binary_key(A, S)
    for r in range(3):
        want = [sum((1 if c >= t else -1) * int(A[r, (c - t) % 64]) for t in range(64) if S[t]) % (1 << 64) for c in range(64)]
        assert got[r].tolist() == want


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_host_keys_from_their_definition(case):
    """The host client's keys for the GPU tests' shapes and seeds: residuals from the definition are centred normal noise of
    the parameter set's deviation, from streams that never repeat.  Host and device run the same det_math.h, so this also
    shows before any GPU run that the fixed seeds lie inside every bound."""
    keys = [K.host_keys(case, seed) for seed in case.seeds]
    K.check_inputs(case, keys)
    K.check_keys_from_definition(case, [k[1:] for k in keys], "host")


@pytest.mark.parametrize("p", [O.TOY_K1, O.TOY_K2], ids=lambda p: p.name)
def test_oracle_keys_from_their_definition(p):
    """The same residual functions on the keys of the one independent key generator in the tree."""
    case = K.BY_NAME[p.name]
    keys = []
    for seed in case.seeds:
        ck = O.ClientKey(p, seed)
        sk = O.ServerKey(ck, fourier=False)
        keys.append((ck.glwe_sk, ck.small_sk, X.ggsw_bits(p, ck.small_sk, 1), sk.bsk, sk.ksk))
    K.check_keys_from_definition(case, keys, "oracle")
