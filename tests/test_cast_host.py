"""Casting keys on the CPU (csrc/cast.cpp, csrc/client.cpp): the host keyswitch against exact integers word for word,
cast_rshift on the reference's four pairs, the reference's decrypt tables on toy twins whose lookups run on the oracle, the
refusals, and the noise model against the variance measured on the host.  The device side is tests/test_gpu_cast.py."""
import dataclasses

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from exact_cast import TO_BIG, TO_SMALL, cast_exact, cast_int, edge_cts, edge_key


def _f():
    import fhestr
    return fhestr


ODD = O.Params(5, 1, 101, 10, 1, 4, 2, 2, 2, 1e-12, 1e-15, "ODD_N101_K1")        # k N = 101: no multiple of any 2 epg
# the reference's key_switching_key/test.rs, restated as data: (source, destination, cast_rshift)
RSHIFT_PAIRS = [("PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_2_CARRY_2_KS_PBS", 2),
                ("PARAM_MESSAGE_1_CARRY_1_KS_PBS", (8, 8), 4),
                ("PARAM_MESSAGE_1_CARRY_1_KS_PBS", "PARAM_MESSAGE_1_CARRY_1_KS_PBS", 0),
                ("PARAM_MESSAGE_2_CARRY_2_KS_PBS", "PARAM_MESSAGE_1_CARRY_1_KS_PBS", -2)]
# its decrypt tables: source value -> (message, carry) the destination's client reads
WIDEN_1_1_TO_2_2 = {0: (0, 0), 1: (1, 0), 2: (2, 0), 3: (3, 0)}                  # 2 * 1 + 1 = 3 is the overflow case
TRUNCATE_2_2_TO_1_1 = {0: (0, 0), 1: (1, 0), 2: (0, 1), 3: (1, 1), 12: (0, 0)}


@pytest.mark.parametrize("src,dst,pair,target,count", [
    (O.TOY_K2, O.TOY_K1, (4, 3), TO_SMALL, 37), (O.TOY_K2, O.TOY_K1, (1, 15), TO_BIG, 20), (O.TOY_K1, O.TOY_K2, (3, 5), TO_BIG, 33),
    (ODD, O.TOY_K2, (1, 16), TO_SMALL, 17), (ODD, O.TOY_K1, (7, 2), TO_BIG, 15), (O.TOY_K1, O.TOY_K1, (4, 4), TO_SMALL, 1)],
    ids=["K2-K1-small-4x3", "K2-K1-big-1x15", "K1-K2-big-3x5", "odd-K2-small-1x16", "odd-K1-big-7x2", "K1-K1-small-one"])
def test_host_loop_equals_exact(src, dst, pair, target, count):
    f = _f()
    rng = np.random.default_rng([src.N, dst.N, pair[0], pair[1], target, count])
    key = edge_key(src, dst, pair, target, rng)
    cts = edge_cts(src, dst, pair, target, rng, count)
    cp = f.cast_default_params(to_fhestr_params(src), to_fhestr_params(dst), target, pair)
    assert f.cast_key_len(to_fhestr_params(dst), cp) == key.size
    got = f.cast_host(to_fhestr_params(dst), cp, key, cts)
    want = cast_exact(src, dst, pair, target, key, cts)
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and not len(bad), f"{len(bad)} of {want.size} words differ; first (row, word) {bad[:8].tolist()}"
    assert np.array_equal(got[0], cast_int(src, dst, pair, target, key, cts[0]))


def test_rshift_of_the_reference_pairs():
    f = _f()

    def params(x):
        return getattr(f, x) if isinstance(x, str) else dataclasses.replace(f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, msg_mod=x[0], carry_mod=x[1])

    assert [f.cast_rshift(params(s), params(d)) for s, d, _ in RSHIFT_PAIRS] == [r for _, _, r in RSHIFT_PAIRS] == [2, 4, 0, -2]


def test_default_params():
    f = _f()
    p11, p22, p44 = f.PARAM_MESSAGE_1_CARRY_1_KS_PBS, f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, to_fhestr_params(O.PARAM_MESSAGE_4_CARRY_4_KS_PBS)
    big = f.cast_default_params(p11, p22, f.CAST_TO_BIG)
    assert (big.base_log, big.level) == (1, 15)                                       # PARAM_KEYSWITCH_1_1_KS_PBS_TO_2_2_KS_PBS
    assert f.cast_key_len(p22, big) == 3 * 512 * 15 * 2049 and f.cast_key_len(p22, big) * 8 == 377_671_680
    small = f.cast_default_params(p11, p22, f.CAST_TO_SMALL)
    assert (small.base_log, small.level) == (p22.ks_base_log, p22.ks_level) and f.cast_key_len(p22, small) == 3 * 512 * 5 * 743
    wide = f.cast_default_params(p22, p44, f.CAST_TO_SMALL)
    assert f.cast_key_len(p44, wide) == 2048 * 7 * 997


def test_refusals():
    f = _f()
    p11, p22, p44 = f.PARAM_MESSAGE_1_CARRY_1_KS_PBS, f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, to_fhestr_params(O.PARAM_MESSAGE_4_CARRY_4_KS_PBS)
    with pytest.raises(f.FheError, match="17 levels, the matrix-core keyswitch takes 1 .. 16"):
        f.cast_default_params(p11, p22, f.CAST_TO_SMALL, (1, 17))
    with pytest.raises(f.FheError, match="base_log 8, the keyswitch digits take 1 .. 7"):
        f.cast_default_params(p11, p22, f.CAST_TO_SMALL, (8, 2))
    with pytest.raises(f.FheError, match=r"the key would hold 8053309440 bytes \(limit 4 GiB\)"):
        f.cast_default_params(p22, p44, f.CAST_TO_BIG)                                # 2048 * 15 * 32769 * 8
    f.cast_default_params(p22, p44, f.CAST_TO_SMALL)
    odd = dataclasses.replace(p22, msg_mod=3, carry_mod=4)
    for s, d in ((odd, p22), (p22, odd)):
        with pytest.raises(f.FheError, match="moduli must be powers of two"):
            f.cast_default_params(s, d, f.CAST_TO_SMALL)
        with pytest.raises(f.FheError, match="moduli must be powers of two"):
            f.cast_rshift(s, d)
    with pytest.raises(f.FheError, match="target"):
        f.cast_default_params(p11, p22, 2)


class _Pair:
    """Two toy clients with library keys, the destination's server key on the oracle, and a casting key between them."""

    def __init__(self, src, dst, target, pair=None, seed=0):
        f = _f()
        self.src, self.dst = src, dst
        self.ck_src, self.ck_dst = f.ClientKey(to_fhestr_params(src), 0xCA570000 + seed), f.ClientKey(to_fhestr_params(dst), 0xCA570100 + seed)
        self.cp, self.key = self.ck_src.gen_cast_key(self.ck_dst, target, pair, seed=0xCA57 + seed)
        self.sk_dst = O.ServerKey.from_keys(dst, *self.ck_dst.gen_server_keys(threads=2))

    def keyswitched(self, cts):
        return _f().cast_host(to_fhestr_params(self.dst), self.cp, self.key, cts)

    def lookup(self, rows, table):
        lut, _ = self.sk_dst.generate_lookup_table(lambda x: int(table[x]))
        if self.cp.target == TO_SMALL:
            return np.stack([self.sk_dst.pbs(r, lut) for r in rows])
        return self.sk_dst.apply_lookup_table_batch(rows, lut)

    def split(self, cts):
        v = self.ck_dst.decrypt(cts)
        return [(int(x) % self.dst.msg_mod, int(x) // self.dst.msg_mod) for x in v]


@pytest.mark.parametrize("target", [TO_BIG, TO_SMALL], ids=["to_big", "to_small"])
def test_widening_table_of_the_reference(target):
    """1_1 -> 2_2 on toy twins (TOY_K2 has the moduli of 1_1, TOY_K1 those of 2_2): 0 .. 3 come out with carry 0, the
    overflow case 2 * 1 + 1 included; the generated key's default pair is the reference's for TO_BIG."""
    f = _f()
    pr = _Pair(O.TOY_K2, O.TOY_K1, target)
    shift = f.cast_rshift(pr.cp.src, to_fhestr_params(pr.dst))
    assert shift == 2
    assert (pr.cp.base_log, pr.cp.level) == ((1, 15) if target == TO_BIG else (O.TOY_K1.ks_base_log, O.TOY_K1.ks_level))
    values = sorted(WIDEN_1_1_TO_2_2)
    cts = pr.ck_src.encrypt(values)
    with np.errstate(over="ignore"):
        cts = np.concatenate([cts, (cts[1:2] * np.uint64(2) + cts[1:2])])             # unchecked_scalar_mul by 2, unchecked_add
    rows = pr.keyswitched(cts)
    out = pr.lookup(rows, [x >> shift for x in range(16)])
    assert pr.split(out) == [WIDEN_1_1_TO_2_2[v] for v in values] + [WIDEN_1_1_TO_2_2[3]]


def test_truncation_table_of_the_reference():
    """2_2 -> 1_1: the source's server key shifts left first ((x << 2) % 16, on the oracle), the keyswitch follows and
    nothing more (shift < 0, TO_BIG): 12 truncates to (0, 0), 3 gives message 1, carry 1."""
    f = _f()
    pr = _Pair(O.TOY_K1, O.TOY_K2, TO_BIG, (4, 4))
    assert f.cast_rshift(pr.cp.src, to_fhestr_params(pr.dst)) == -2
    sk_src = O.ServerKey.from_keys(pr.src, *pr.ck_src.gen_server_keys(threads=2))
    values = sorted(TRUNCATE_2_2_TO_1_1)
    lut, _ = sk_src.generate_lookup_table(lambda x: (x << 2) % 16)
    prepared = sk_src.apply_lookup_table_batch(pr.ck_src.encrypt(values), lut)
    assert pr.split(pr.keyswitched(prepared)) == [TRUNCATE_2_2_TO_1_1[v] for v in values]


def test_same_set_other_key():
    """shift 0, both targets: TO_BIG raw decrypts under the destination's key as it stands, TO_SMALL after the identity table."""
    for target in (TO_BIG, TO_SMALL):
        pr = _Pair(O.TOY_K1, O.TOY_K1, target, (4, 4), seed=1)
        values = list(range(16))
        rows = pr.keyswitched(pr.ck_src.encrypt(values))
        out = rows if target == TO_BIG else pr.lookup(rows, list(range(16)))
        assert [int(x) for x in pr.ck_dst.decrypt(out)] == values
        assert [int(x) for x in pr.ck_src.decrypt(out)] != values, "the source client still reads the cast blocks"


def test_regrouping_degrees():
    """fhe_cast_regroup_check, the rule CastKey::set_group applies: the combined lookup input (msg_src^g - 1) << shift against
    the destination's message-and-carry space for the three widenings of string casts.  1_1 -> 2_2 and 2_2 -> 4_4 fit;
    1_1 -> 4_4 does not (one lookup cannot carry four source blocks: 15 << 6 = 960 > 255)."""
    f = _f()
    p11, p22, p44 = f.PARAM_MESSAGE_1_CARRY_1_KS_PBS, f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, to_fhestr_params(O.PARAM_MESSAGE_4_CARRY_4_KS_PBS)
    assert f.cast_regroup_check(p11, p22, 2) == (12, 16) and f.cast_regroup_check(p22, p44, 2) == (240, 256)
    assert f.cast_regroup_check(p11, p22, 1) == (4, 16) and f.cast_regroup_check(p22, p22, 1) == (3, 16)
    with pytest.raises(f.FheError, match="4 source blocks give a lookup input of up to 960, the destination's message-and-carry space ends at 255"):
        f.cast_regroup_check(p11, p44, 4)
    with pytest.raises(f.FheError, match="2 source blocks do not fill one destination block"):
        f.cast_regroup_check(p11, p44, 2)
    with pytest.raises(f.FheError, match="only a cast to more bits per block regroups"):
        f.cast_regroup_check(p22, p22, 2)
    with pytest.raises(f.FheError, match="only a cast to more bits per block regroups"):
        f.cast_regroup_check(p22, p11, 2)


def _signed(x):
    return np.asarray(x, dtype=np.uint64).astype(np.int64).astype(np.float64)


@pytest.mark.parametrize("target", [TO_BIG, TO_SMALL], ids=["to_big", "to_small"])
def test_noise_matches_the_model(target):
    """(phase of the keyswitched block under the destination's key) - (phase of the source block under the source's) over
    S = 4096 blocks against fhe_cast_noise at v_in = 0: the key-noise and rounding terms of the keyswitch alone.  The
    source has k N = 1024 and the pair four levels, so the 4096 key rows average their own noise to 2 %; destination lwe_std
    2^-20 so that both terms count.  Margins as in tests/test_packing_ks.py: six standard errors of a mean, resp. of a
    variance estimate (relative sqrt(2 / S))."""
    f = _f()
    src = O.Params(16, 1, 1024, 10, 2, 4, 4, 4, 4, 1e-12, 1e-15, "TOY_SRC_N1024")
    dst = dataclasses.replace(O.TOY_K1, lwe_std=2.0**-20, name="TOY_K1_noisy_lwe")
    S, pair = 4096, (4, 4)
    Ps, Pd = to_fhestr_params(src), to_fhestr_params(dst)
    ck_src, ck_dst = f.ClientKey(Ps, 0xCA570300), f.ClientKey(Pd, 0xCA570301)
    cp, key = ck_src.gen_cast_key(ck_dst, target, pair, seed=17)
    cts = ck_src.encrypt(np.arange(S) % 16)
    rows = f.cast_host(Pd, cp, key, cts)
    big_src, _ = ck_src.secret_keys()
    big_dst, small_dst = ck_dst.secret_keys()
    sk_out = small_dst if target == TO_SMALL else big_dst
    with np.errstate(over="ignore"):
        diff = _signed((rows[:, -1] - rows[:, :-1] @ sk_out) - (cts[:, -1] - cts[:, :-1] @ big_src)) / 2.0**64
    model = f.cast_noise(Pd, cp, 0.0)[2]
    mean, var = diff.mean(), diff.var()
    print(f"cast noise ({'small' if target else 'big'}): mean {mean:.3e} (sd / sqrt(S) = {np.sqrt(var / S):.3e}), variance {var:.4e}, model {model:.4e}, "
          f"ratio {var / model:.4f}, margin {6 * np.sqrt(2 / S):.4f}")
    assert abs(mean) <= 6 * np.sqrt(var / S)
    assert abs(var / model - 1) <= 6 * np.sqrt(2 / S)
    nominal, budget, torus = f.cast_noise(Pd, cp, 1.0)
    assert torus > model and budget > 0 and nominal > 0
