"""Ring packing on the CPU (csrc/ring_packing.cpp): the host reference against the definition in Python integers
(tests/exact_ring_packing.py) word for word, decryption, the host transform, the parameter table and its bounds, and the
noise model against the host reference.  The device side is tests/test_gpu_ring_packing.py; the same units under
AddressSanitizer + UBSan are tests/test_ring_packing_host.py."""
import math

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
import exact_ring_packing as X


def _f():
    import fhestr
    return fhestr


def toy(k, N, glwe_std=1e-15, msg=2, carry=2):
    return O.Params(4, k, N, 10, 1, 4, 2, msg, carry, 1e-12, glwe_std, f"RING_TOY_K{k}_N{N}")


def counts_of(N):
    return [1, 2, 3, N - 1, N, N + 1]


# (shape, the two pairs): N = 16 and 64 with k = 1, a k = 2 and a k = 3 toy shape
WORD_CASES = [(toy(1, 16), (8, 4), counts_of(16)), (toy(1, 16), (3, 7), counts_of(16)),
              (toy(1, 64), (6, 4), counts_of(64)), (toy(1, 64), (11, 2), [3, 65]),
              (toy(2, 16), (5, 3), counts_of(16)), (toy(2, 16), (9, 2), [3, 17]),
              (toy(3, 8), (4, 5), counts_of(8)), (toy(3, 8), (10, 2), [3, 9])]


@pytest.mark.parametrize("p,pair,counts", WORD_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_host_reference_equals_the_definition(p, pair, counts):
    f = _f()
    P = to_fhestr_params(p)
    rng = np.random.default_rng([p.k, p.N, pair[0], pair[1]])
    key = X.edge_key(p, pair, rng)
    assert key.size == f.ring_packing_key_len(P, pair) == (p.N.bit_length() - 1) * p.k * pair[1] * (p.k + 1) * p.N
    for count in counts:
        cts = rng.integers(0, 2**64, size=(count, p.k * p.N + 1), dtype=np.uint64)
        cts[0, :4] = [0, 2**64 - 1, 2**63, 2**63 - 1]          # the division's and the decomposer's edges
        want = X.ring_pack_int(p, pair, key, cts)
        got = f.ring_pack_host(P, pair, key, cts)
        assert got.shape == want.shape == (-(-count // p.N), p.k + 1, p.N)
        bad = np.argwhere(got != want)
        assert not len(bad), f"count {count}: {len(bad)} of {want.size} words differ; first (glwe, polynomial, coefficient) {bad[:8].tolist()}"


def _phases(f, ck, P, glwes):
    """body - sum_q A_q S_q of every GLWE, as signed torus values [G, N]."""
    sk, _ = ck.secret_keys()
    out = []
    for g in np.asarray(glwes, dtype=np.uint64).reshape(-1, P.k + 1, P.N):
        ph = [int(v) for v in g[P.k]]
        for q in range(P.k):
            prod = X.negacyclic([int(v) for v in g[q]], [int(v) for v in sk[q * P.N:(q + 1) * P.N]])
            ph = [a - b for a, b in zip(ph, prod)]
        out.append([((v + 2**63) % 2**64 - 2**63) / 2.0**64 for v in ph])
    return np.array(out)


@pytest.mark.parametrize("p,pair", [(toy(1, 64), (8, 4)), (toy(2, 16), (7, 4)), (toy(3, 8), (6, 5))], ids=lambda v: getattr(v, "name", str(v)))
def test_packed_coefficients_decrypt(p, pair):
    f = _f()
    P = to_fhestr_params(p)
    ck = f.ClientKey(P, 0x5EED0D00 + p.N)
    pair, key = ck.gen_ring_packing_key(pair, seed=3)
    M = p.msg_mod * p.carry_mod
    for count in (1, 3, p.N - 1, p.N, p.N + 1):
        msgs = (np.arange(count) * 3 + 1) % M
        glwes = f.ring_pack_host(P, pair, key, ck.encrypt(msgs))
        assert np.array_equal(ck.decrypt_packed(glwes, count), msgs)
        # the unused coefficients of a short group hold no message: their phase is 0 within the noise
        used = count % p.N or p.N
        tail = _phases(f, ck, P, glwes)[-1][used:]
        assert np.all(np.abs(tail) < 6 * math.sqrt(X.variance(p, pair)) + 2.0**-40), np.abs(tail).max(initial=0)
    ck.close()


def test_key_generation_is_seeded_and_thread_independent():
    f = _f()
    P = to_fhestr_params(toy(2, 16))
    ck = f.ClientKey(P, 5)
    a = ck.gen_ring_packing_key((5, 3), seed=9, threads=1)[1]
    b = ck.gen_ring_packing_key((5, 3), seed=9, threads=7)[1]
    c = ck.gen_ring_packing_key((5, 3), seed=10, threads=1)[1]
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    ck.close()


# ---- the host transform ---------------------------------------------------------------------------------------------------
def _convolve(a, b):
    """sum_t a[t] (*) b[t], negacyclic, numpy int64."""
    N = a.shape[1]
    out = np.zeros(N, dtype=np.int64)
    for x, y in zip(a.astype(np.int64), b.astype(np.int64)):
        full = np.concatenate([np.convolve(x, y), [0]])
        out += full[:N] - full[N:]
    return out


@pytest.mark.parametrize("N", [4, 64, 2048, 32768])
def test_transform_round_trip(N):
    f = _f()
    a = np.random.default_rng(N).integers(0, X.P, size=(3, N), dtype=np.uint32)
    a[0, :2] = [0, X.P - 1]
    fwd = f.ring_ntt_host(a)
    assert not np.array_equal(fwd, a) and fwd.max() < X.P
    assert np.array_equal(f.ring_ntt_host(fwd, inverse=True), a)


@pytest.mark.parametrize("N", [64, 2048])
def test_product_equals_schoolbook(N):
    rng = np.random.default_rng(N + 1)
    a = rng.integers(-2**11, 2**11 + 1, size=(2, N))
    b = rng.integers(-128, 128, size=(2, N))
    assert np.array_equal(_f().ring_product_host(a, b), _convolve(a, b))


def test_all_extreme_product_at_the_prime_bound():
    """N = 32768, every digit -2^(b-1) and every plane word -128 at the largest admitted L 2^(b-1) = 7 * 64, the pair (7, 7):
    coefficient N - 1 of the sum is 7 * 2^28, 0.875 of P / 2 (PARAM_MESSAGE_4_CARRY_4's own pair (7, 5) reaches 5 * 2^28).
    A lift that is not centred, or centred on the wrong side, fails here and nowhere else."""
    N, L, b = 32768, 7, 7
    admitted = [(bb, ll) for bb in range(1, 33) for ll in range(1, 17) if bb * ll <= 63 and X.prime_bound_ok(toy(1, N), (bb, ll))]
    assert max(ll * 2**(bb - 1) for bb, ll in admitted) == L * 2**(b - 1)
    a = np.full((L, N), -2**(b - 1), dtype=np.int64)
    pl = np.full((L, N), -128, dtype=np.int64)
    want = _convolve(a, pl)
    assert want.max() == L * 2**(b - 1) * 128 * N > 0.87 * (X.P // 2) and want.min() < -0.87 * (X.P // 2)
    assert np.array_equal(_f().ring_product_host(a, pl), want)


# ---- parameters -----------------------------------------------------------------------------------------------------------
# what fhe_ring_packing_default_params returns, per parameter set the library names (DESIGN.md section 3 lists the same)
DEFAULTS = {"PARAM_MESSAGE_1_CARRY_1_KS_PBS": (13, 2), "PARAM_MESSAGE_2_CARRY_1_KS_PBS": (12, 2), "PARAM_MESSAGE_2_CARRY_2_KS_PBS": (12, 2),
            "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS": (13, 2), "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS": (13, 2),
            "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS": (12, 2), "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS": (12, 2),
            "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS": (10, 3), "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS": (10, 3),
            "PARAM_MESSAGE_4_CARRY_4_KS_PBS": (7, 5)}


def _sets():
    f = _f()
    return [getattr(f, n) for n in sorted(dir(f)) if n.startswith("PARAM_")]


def _log2_pfail(half_box, variance):
    z = half_box / math.sqrt(variance)
    p = math.erfc(z / math.sqrt(2.0))
    return math.log2(p) if p > 1e-300 else (-(z * z) / 2 - math.log(z * math.sqrt(math.pi / 2))) / math.log(2.0)


def test_default_params_per_set():
    f = _f()
    assert {P.name for P in _sets()} == set(DEFAULTS)
    for P in _sets():
        got = f.ring_packing_default_params(P)
        words = f.ring_packing_key_len(P, got)
        print(f"ring packing default {P.name}: base_log {got[0]}, level {got[1]}, key {words * 8} bytes")
        assert got == DEFAULTS[P.name]
        assert words == (P.N.bit_length() - 1) * P.k * got[1] * (P.k + 1) * P.N
    assert f.ring_packing_key_len(f.PARAM_MESSAGE_4_CARRY_4_KS_PBS, (7, 5)) * 8 == 39321600
    assert f.ring_packing_key_len(f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, (12, 2)) * 8 < 1 << 20
    # the N = 16384 shapes the matrix route refuses have a pair too
    for p in (q for q in O.TOY_SHAPES if q.N == 16384):
        pair = f.ring_packing_default_params(to_fhestr_params(p))
        assert f.ring_packing_key_len(to_fhestr_params(p), pair) > 0


def test_default_params_are_the_cheapest_under_both_bounds():
    """The failure bound recomputed from fhe_noise_model, as tests/test_packing_ks.py does for the matrix route, with
    exact_ring_packing.variance: the returned pair meets it under the one-prime bound; every cheaper pair -- fewer levels
    with any base, or the same levels with a larger base -- misses the decode bound or the prime bound."""
    f = _f()
    for P in _sets() + [to_fhestr_params(O.TOY_K1)]:
        m = f.noise_model(P)
        safety = 1.0 if f.noise_model_is_calibrated(P) else 4.0
        max_level = (P.msg_mod * P.carry_mod - 1) / max(1, P.msg_mod - 1)
        target = _log2_pfail(m["half_box"], max_level**2 * safety * m["v_pbs"] + m["v_ks"] + m["v_ms"]) + (0.0 if P.grouping == 2 else 0.5)
        pfail = lambda pair: _log2_pfail(m["half_box"], safety * m["v_pbs"] + X.variance(P, pair))
        base_log, level = f.ring_packing_default_params(P)
        assert X.prime_bound_ok(P, (base_log, level)) and pfail((base_log, level)) <= target
        cheaper = [(b, l) for l in range(1, level) for b in range(1, 33)] + [(b, level) for b in range(base_log + 1, 33)]
        for pair in cheaper:
            if pair[0] * pair[1] <= 63:
                assert not X.prime_bound_ok(P, pair) or pfail(pair) > target, (P.name, pair)


@pytest.mark.parametrize("P_name,pair", [("PARAM_MESSAGE_4_CARRY_4_KS_PBS", (8, 5)), ("PARAM_MESSAGE_4_CARRY_4_KS_PBS", (7, 8)),
                                         ("PARAM_MESSAGE_2_CARRY_2_KS_PBS", (13, 2)), ("PARAM_MESSAGE_2_CARRY_2_KS_PBS", (12, 4))], ids=str)
def test_pairs_over_the_prime_bound_are_refused(P_name, pair):
    f = _f()
    P = getattr(f, P_name)
    assert not X.prime_bound_ok(P, pair)
    assert f.ring_packing_key_len(P, pair) == 0
    assert "one-prime bound" in f.lib().fhe_last_error().decode()
    with pytest.raises(f.FheError, match="one-prime bound"):
        f.ring_packing_noise(P, pair)
    with pytest.raises(f.FheError, match="one-prime bound"):
        f.ring_pack_host(P, pair, np.zeros(8, dtype=np.uint64), np.zeros((1, P.big_size), dtype=np.uint64))


@pytest.mark.parametrize("pair", [(0, 1), (33, 1), (1, 0), (1, 17), (8, 8), (4, 16)], ids=str)
def test_out_of_range_decompositions_are_refused(pair):
    f = _f()
    P = to_fhestr_params(toy(1, 16))
    assert f.ring_packing_key_len(P, pair) == 0
    ck = f.ClientKey(P, 1)
    with pytest.raises(f.FheError, match="unsupported ring packing decomposition"):
        ck.gen_ring_packing_key(pair)
    ck.close()


def test_cost_formula():
    f = _f()
    assert f.ring_pack_keyswitches(f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 1024) == X.keyswitch_count(2048, 1024) == 2047
    assert f.ring_pack_keyswitches(f.PARAM_MESSAGE_4_CARRY_4_KS_PBS, 2048) == X.keyswitch_count(32768, 2048) == 10239
    assert f.ring_pack_keyswitches(f.PARAM_MESSAGE_4_CARRY_4_KS_PBS, 3) == X.keyswitch_count(32768, 3) == 42
    assert f.ring_pack_keyswitches(f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 2049) == 2047 + 11


def test_noise_model_matches_exact_variance():
    f = _f()
    for P in _sets():
        pair = f.ring_packing_default_params(P)
        nominal, budget = f.ring_packing_noise(P, pair)
        m = f.noise_model(P)
        assert nominal == pytest.approx(1.0 + X.variance(P, pair) / m["v_pbs"], rel=1e-9)
        wide = f.ring_narrow_noise(P, pair, 32)
        assert wide[0] == pytest.approx(nominal, rel=1e-6) and wide[1] == budget
        assert f.ring_narrow_noise(P, pair, 8)[0] > wide[0]


# ---- noise: the host reference against the model -------------------------------------------------------------------------------
# (shape, pair, GLWEs): 4,096 packed coefficients each, the rounding term ruling as on the named sets
NOISE_CASES = [(toy(1, 64), (4, 3), 64), (toy(2, 32), (5, 2), 128)]
# measured / modelled variance of these exact runs (profiles/ring_packing.txt); the band is that figure with the 3 sigma of
# 4,096 samples, 3 sqrt(2 / 4096) = 6.6 %, on either side
NOISE_MEASURED = {"RING_TOY_K1_N64": 0.986, "RING_TOY_K2_N32": 1.133}
NOISE_BAND = 3 * math.sqrt(2 / 4096)


def measured_over_modelled(p, pair, glwes_n):
    f = _f()
    P = to_fhestr_params(p)
    ck = f.ClientKey(P, 0x5EED0E00 + p.N)
    pair, key = ck.gen_ring_packing_key(pair, seed=11)
    count = glwes_n * p.N
    glwes = f.ring_pack_host(P, pair, key, ck.encrypt(np.zeros(count, dtype=np.int64)))
    err = _phases(f, ck, P, glwes).reshape(-1)
    ck.close()
    assert err.size >= 4096
    return float(np.mean(err**2)) / (X.variance(p, pair) + p.glwe_std**2)


@pytest.mark.parametrize("p,pair,glwes_n", NOISE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_noise_follows_the_model(p, pair, glwes_n):
    ratio = measured_over_modelled(p, pair, glwes_n)
    print(f"ring packing noise {p.name} {pair}: measured / modelled variance {ratio:.3f}")
    centre = NOISE_MEASURED[p.name]
    assert centre * (1 - NOISE_BAND) <= ratio <= centre * (1 + NOISE_BAND)
    assert 2**-0.4 <= centre <= 2**0.4              # the model itself: within 2^0.2 in standard deviation


def test_wire_round_trip():
    f = _f()
    from fhestr import wire
    P = to_fhestr_params(toy(2, 16))
    ck = f.ClientKey(P, 21)
    pair, key = ck.gen_ring_packing_key((5, 3), seed=4)
    data = wire.write_ring_packing_key(P, pair, key)
    assert len(data) > 8 + key.nbytes + 4 * 8                # the length, the data, four dimensions, then the modulus
    got_pair, got_key = wire.read_ring_packing_key(P, data)
    assert got_pair == pair and np.array_equal(got_key, key)
    with pytest.raises(f.FheError, match="truncated"):
        wire.read_ring_packing_key(P, data[:-3])
    with pytest.raises(f.FheError, match="does not match the parameter set"):
        wire.read_ring_packing_key(to_fhestr_params(toy(1, 16)), data)
    with pytest.raises(f.FheError):
        wire.read_packing_key(P, data)                      # the matrix key's reader wants another length
    ck.close()
