"""The packing keyswitch on the CPU: the exact reference against itself, the library's host loop against it word for word,
key generation, decryption, noise, and the parameter checks (csrc/client.cpp).  The device side is
tests/test_gpu_packing_ks.py."""
import dataclasses

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from exact_packing import ExactPacking, as_keyswitch_shape, edge_pack_cts, edge_pksk, pack_exact, pack_int, sparse_case


def _f():
    import fhestr
    return fhestr


TINY = O.Params(4, 1, 32, 10, 1, 4, 2, 2, 2, 1e-12, 1e-15, "TINY_N32_K1")
TINY_K2 = O.Params(4, 2, 32, 10, 1, 4, 2, 2, 2, 1e-12, 1e-15, "TINY_N32_K2")


@pytest.mark.parametrize("p,pp,count", [(TINY, (4, 2), 33), (TINY, (7, 2), 32), (TINY_K2, (3, 5), 35), (TINY, (1, 16), 5)],
                         ids=["k1-4x2-N+1", "k1-7x2-N", "k2-3x5-N+3", "k1-1x16"])
def test_batched_form_equals_the_integer_form(p, pp, count):
    rng = np.random.default_rng([p.k, pp[0], pp[1], count])
    key = edge_pksk(p, pp, rng)
    cts = edge_pack_cts(p, pp, rng, count)
    want = pack_int(p, pp, key, cts)
    got = pack_exact(p, pp, key, cts)
    assert got.shape == want.shape == (-(-count // p.N), p.k + 1, p.N)
    assert np.array_equal(got, want)


def test_rotation_by_hand():
    """One LWE with a zero mask at position d: the body lands at coefficient d of polynomial k and nowhere else."""
    p, pp = TINY, (4, 2)
    key = np.random.default_rng(1).integers(0, 2**64, size=(p.k * p.N * pp[1], p.k + 1, p.N), dtype=np.uint64)
    cts = np.zeros((p.N + 3, p.k * p.N + 1), dtype=np.uint64)
    cts[:, -1] = np.arange(1, p.N + 4, dtype=np.uint64)
    want = np.zeros((2, p.k + 1, p.N), dtype=np.uint64)
    want[0, p.k, :] = np.arange(1, p.N + 1)
    want[1, p.k, :3] = np.arange(p.N + 1, p.N + 4)
    for got in (pack_int(p, pp, key, cts), pack_exact(p, pp, key, cts), _f().packing_keyswitch_host(to_fhestr_params(p), pp, key, cts)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("p,pp,count", [(O.TOY_K1, (4, 3), 257), (O.TOY_K2, (7, 2), 129), (O.TOY_K2, (3, 5), 50), (TINY, (1, 16), 33)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_host_loop_equals_exact(p, pp, count):
    rng = np.random.default_rng([p.N, p.k, pp[0], pp[1], count])
    key = edge_pksk(p, pp, rng)
    cts = edge_pack_cts(p, pp, rng, count)
    got = _f().packing_keyswitch_host(to_fhestr_params(p), pp, key, cts)
    want = pack_exact(p, pp, key, cts)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} of {want.size} words differ; first (glwe, polynomial, coefficient) {bad[:8].tolist()}"


def _negacyclic(s):
    """M with (a @ M)[c'] = (a * s)[c'] in Z[X] / (X^N + 1), uint64."""
    N = len(s)
    m = np.zeros((N, N), dtype=np.uint64)
    for t in np.nonzero(s)[0]:
        for c in range(N):
            if c + t < N:
                m[c, c + t] += np.uint64(1)
            else:
                m[c, c + t - N] -= np.uint64(1)
    return m


def _glwe_phases(p, glwe_sk, glwes):
    """body - sum_q A_q S_q of [G, k + 1, N] GLWEs: [G, N] uint64."""
    glwes = np.asarray(glwes, dtype=np.uint64).reshape(-1, p.k + 1, p.N)
    ph = glwes[:, p.k, :].copy()
    with np.errstate(over="ignore"):
        for q in range(p.k):
            ph -= glwes[:, q, :] @ _negacyclic(glwe_sk[q * p.N:(q + 1) * p.N])
    return ph


def _signed(x):
    return np.asarray(x, dtype=np.uint64).astype(np.int64).astype(np.float64)


@pytest.mark.parametrize("p,pp", [(O.TOY_K1, (4, 3)), (O.TOY_K2, (7, 2))], ids=["TOY_K1-4x3", "TOY_K2-7x2"])
def test_generated_key_encrypts_the_key_bits(p, pp):
    """Row (i, l) decrypts to s_i << (64 - base_log l) in coefficient 0 and to 0 elsewhere, within 8 sigma of glwe_std."""
    P = to_fhestr_params(p)
    ck = _f().ClientKey(P, 0x5EED0100 + p.k)
    got_pp, key = ck.gen_packing_key(pp, seed=7, threads=3)
    assert got_pp == pp and key.size == _f().packing_key_len(P, pp) == p.k * p.N * pp[1] * (p.k + 1) * p.N
    again = ck.gen_packing_key(pp, seed=7, threads=1)[1]
    assert np.array_equal(key, again), "the key depends on the thread count"
    glwe_sk, _ = ck.secret_keys()
    ph = _glwe_phases(p, glwe_sk, key).reshape(p.k * p.N, pp[1], p.N)
    want = np.zeros_like(ph)
    for it in range(pp[1]):
        want[:, it, 0] = glwe_sk << np.uint64(64 - pp[0] * (pp[1] - it))       # level L first
    err = np.abs(_signed(ph - want))
    bound = 8 * p.glwe_std * 2.0**64
    assert err.max() <= bound, f"largest error {err.max():.0f} > 8 sigma = {bound:.0f}"
    assert err.max() > 0, "no noise at all"
    ck.close()


@pytest.mark.parametrize("count", [1, 256, 257], ids=["one", "N", "N+1"])
def test_round_trip(count):
    p = O.TOY_K1
    P = to_fhestr_params(p)
    ck = _f().ClientKey(P, 0x5EED0200)
    pp, key = ck.gen_packing_key(seed=11)
    assert pp == _f().packing_default_params(P)
    msgs = (np.arange(count) * 7 + 3) % (p.msg_mod * p.carry_mod)
    cts = ck.encrypt(msgs)
    glwes = _f().packing_keyswitch_host(P, pp, key, cts)
    assert glwes.shape == (-(-count // p.N), p.k + 1, p.N) and glwes.size == _f().packed_glwe_len(P, count)
    assert np.array_equal(ck.decrypt_packed(glwes, count), msgs)
    assert np.array_equal(ck.decrypt(cts), msgs)
    with pytest.raises(_f().FheError):
        ck.decrypt_packed(glwes.reshape(-1)[:-1], count)
    ck.close()


def test_noise_matches_the_model():
    """(phase error of packed coefficient j) - (phase error of input LWE j) over S = 4096 coefficients (16 full GLWEs of the
    N = 256 toy set, GLWE noise raised to 2^-20 so that both terms of the model count).  Model, evaluated on the actual key
    and digits: the rounding of LWE j's mask against the key bits, hw(s) 2^(-2 base_log level) / 12, plus one key-noise
    coefficient per digit of EVERY LWE of the same GLWE (the rotation only moves them): glwe_var * sum digit^2 over the
    group.  Margins: six standard errors of a mean, resp. of a variance estimate (relative sqrt(2 / S))."""
    p = dataclasses.replace(O.TOY_K1, glwe_std=2.0**-20, name="TOY_K1_noisy")
    pp, S = (4, 3), 4096
    P = to_fhestr_params(p)
    ck = _f().ClientKey(P, 0x5EED0300)
    _, key = ck.gen_packing_key(pp, seed=13)
    glwe_sk, _ = ck.secret_keys()
    cts = ck.encrypt(np.arange(S) % (p.msg_mod * p.carry_mod))
    glwes = _f().packing_keyswitch_host(P, pp, key, cts)
    with np.errstate(over="ignore"):
        lwe_phase = cts[:, -1] - cts[:, :-1] @ glwe_sk
        diff = _signed(_glwe_phases(p, glwe_sk, glwes).reshape(-1)[:S] - lwe_phase) / 2.0**64
    digits = ExactPacking(p, pp, key).ks.digits(cts).astype(np.float64)
    per_group = (digits**2).sum(axis=1).reshape(-1, p.N).sum(axis=1)            # sum digit^2 of every GLWE's LWEs
    model = int(glwe_sk.sum()) * 2.0**(-2 * pp[0] * pp[1]) / 12 + p.glwe_std**2 * per_group.mean()
    mean, var = diff.mean(), diff.var()
    print(f"packing noise: mean {mean:.3e} (sd / sqrt(S) = {np.sqrt(var / S):.3e}), variance {var:.4e}, model {model:.4e}, "
          f"ratio {var / model:.4f}, margin {6 * np.sqrt(2 / S):.4f}")
    assert abs(mean) <= 6 * np.sqrt(var / S)
    assert abs(var / model - 1) <= 6 * np.sqrt(2 / S)
    ck.close()


def _log2_pfail(half_box, variance):
    """NoiseModel::log2_pfail (csrc/noise_model.h): two-sided Gaussian tail beyond half a box."""
    import math
    z = half_box / math.sqrt(variance)
    p = math.erfc(z / math.sqrt(2.0))
    if p > 1e-300:
        return math.log2(p)
    return (-(z * z) / 2 - math.log(z * math.sqrt(math.pi / 2))) / math.log(2.0)


def _packing_pfail(P, m, safety, pp):
    """log2 failure probability of a packed PBS output decoded at delta / 2: one nominal variance, one key-noise
    coefficient per digit of each of the N LWEs of the GLWE, the rounding of its own mask against k N / 2 key bits."""
    base_log, level = pp
    kN, B = P.k * P.N, 2.0**base_log
    pack = P.N * kN * level * (B * B + 2) / 12 * P.glwe_std**2 + kN / 2 / 12 * 2.0**(-2 * base_log * level)
    return _log2_pfail(m["half_box"], safety * m["v_pbs"] + pack)


def _sets():
    f = _f()
    return [getattr(f, n) for n in sorted(dir(f)) if n.startswith("PARAM_")]


# what fhe_packing_default_params returns, per parameter set the library names (DESIGN.md section 3 lists the same)
DEFAULTS = {"PARAM_MESSAGE_1_CARRY_1_KS_PBS": (7, 2), "PARAM_MESSAGE_2_CARRY_1_KS_PBS": (7, 2), "PARAM_MESSAGE_2_CARRY_2_KS_PBS": (7, 2),
            "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS": (7, 2), "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS": (7, 2),
            "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS": (7, 2), "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS": (7, 2),
            "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS": (7, 3), "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS": (7, 3),
            "PARAM_MESSAGE_4_CARRY_4_KS_PBS": None}


def test_default_params_per_set():
    f = _f()
    assert {P.name for P in _sets()} == set(DEFAULTS)
    for P in _sets():
        want = DEFAULTS[P.name]
        if want is None:                                    # N = 32768: any pair that decodes needs a key above 4 GiB
            with pytest.raises(f.FheError, match="unsupported parameter set"):
                f.packing_default_params(P)
            continue
        got = f.packing_default_params(P)
        words = f.packing_key_len(P, got)
        print(f"packing default {P.name}: base_log {got[0]}, level {got[1]}, key {words * 8} bytes")
        assert got == want
        assert words == P.k * P.N * got[1] * (P.k + 1) * P.N and words * 8 <= 1 << 32
    for p in (O.TOY_K1, O.TOY_K2):
        assert f.packing_default_params(to_fhestr_params(p)) == (7, 2)


def test_default_params_are_the_cheapest_that_meet_the_plan_bound():
    """The bound recomputed from fhe_noise_model: the failure probability a plan tolerates at a PBS input of the
    reference-shaped worst case nu = max_noise_level^2, half a bit of slack (none at grouping factor 2), V_pbs times four on
    shapes whose model is unmeasured (default_noise_budget).  The returned pair meets it; every cheaper pair -- fewer levels
    with any base, or the same levels with a larger base -- misses it."""
    f = _f()
    for P in _sets() + [to_fhestr_params(O.TOY_K1)]:
        if DEFAULTS.get(P.name, 0) is None:
            continue
        m = f.noise_model(P)
        safety = 1.0 if f.noise_model_is_calibrated(P) else 4.0
        max_level = (P.msg_mod * P.carry_mod - 1) / max(1, P.msg_mod - 1)
        target = _log2_pfail(m["half_box"], max_level**2 * safety * m["v_pbs"] + m["v_ks"] + m["v_ms"]) + (0.0 if P.grouping == 2 else 0.5)
        base_log, level = f.packing_default_params(P)
        got = _packing_pfail(P, m, safety, (base_log, level))
        cheaper = [(b, l) for l in range(1, level) for b in range(1, 8)] + [(b, level) for b in range(base_log + 1, 8)]
        worst = min((_packing_pfail(P, m, safety, pp), pp) for pp in cheaper)
        print(f"packing bound {P.name}: target 2^{target:.1f}; ({base_log}, {level}) 2^{got:.1f}; best cheaper pair {worst[1]} 2^{worst[0]:.1f}")
        assert got <= target
        assert worst[0] > target


def test_n8192_three_level_key_on_the_host():
    """PARAM_MULTI_BIT_MESSAGE_3_CARRY_3's default (7, 3): the 3.2 GB key.  Only the key rows of the mask elements that are
    not zero are ever read (zero elements have zero digits), so the key is allocated untouched and those rows alone are
    filled; the reference is the formula on the same rows, in wrapping uint64."""
    p, pp = O.TOY_N8192, (7, 3)
    assert _f().packing_default_params(_f().PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS) == pp
    key, cts, want = sparse_case(p, pp, 37)
    got = _f().packing_keyswitch_host(to_fhestr_params(p), pp, key, cts)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pp", [(0, 1), (8, 1), (1, 0), (1, 17), (7, 10), (4, 16)], ids=str)
def test_out_of_range_decompositions_are_refused(pp):
    f = _f()
    P = to_fhestr_params(O.TOY_K1)
    assert f.packing_key_len(P, pp) == 0
    ck = f.ClientKey(P, 1)
    with pytest.raises(f.FheError, match="unsupported packing decomposition"):
        ck.gen_packing_key(pp)
    with pytest.raises(f.FheError):
        f.packing_keyswitch_host(P, pp, np.zeros(8, dtype=np.uint64), np.zeros((1, P.big_size), dtype=np.uint64))
    ck.close()


def test_accepted_extremes():
    P = to_fhestr_params(O.TOY_K1)
    for pp in ((7, 9), (1, 16), (7, 1), (3, 16)):
        assert _f().packing_key_len(P, pp) == 256 * pp[1] * 512


@pytest.mark.parametrize("p", [O.TOY_N32768, O.PARAM_MESSAGE_4_CARRY_4_KS_PBS, next(q for q in O.TOY_SHAPES if q.N == 16384)],
                         ids=lambda p: p.name)
def test_oversized_parameter_sets_are_refused(p):
    """N >= 16384: the key of any pair that decodes exceeds 4 GiB.  The documented answer: key length 0, the call fails with
    the unsupported-parameter message."""
    f = _f()
    P = to_fhestr_params(p)
    assert f.packing_key_len(P, (7, 2)) == 0
    assert "unsupported parameter set" in f.lib().fhe_last_error().decode()
    with pytest.raises(f.FheError, match="unsupported parameter set"):
        f.packing_default_params(P)
    ck = f.ClientKey(to_fhestr_params(dataclasses.replace(p, n=4)), 1)
    with pytest.raises(f.FheError, match="unsupported parameter set"):
        ck.gen_packing_key((7, 2))
    ck.close()
