"""The shapes at which generated server keys are checked from their definition (tests/exact_keys.py), shared by the CPU
tests on the host client's keys (test_exact_keys.py) and the GPU tests on the device's (test_gpu_exact_keys.py): each is
the smallest at which that part of bsk_gen_kernel / ksk_gen_kernel can differ.  Secret keys are the host client's for the
listed seeds; the seeds were chosen so that the preconditions of `check_inputs` hold, and every test asserts them."""
import dataclasses

import numpy as np

import oracle as O
import exact_keys as X


@dataclasses.dataclass(frozen=True)
class Case:
    params: object              # oracle.Params
    grouping: int               # 1 = classic PBS
    seeds: tuple
    reaches: str
    per_bit: int = None         # residuals on the first and the last GGSW and up to per_bit more of each plaintext bit (None: all)

    @property
    def name(self):
        return self.params.name

    @property
    def n_ggsw(self):
        p, g = self.params, self.grouping
        return p.n if g <= 1 else p.n // g * (1 << g)


def _shape(name):
    return next(p for p in O.TOY_SHAPES if p.name == name)


CASES = [
    Case(O.TOY_K2, 1, (0x4B450101, 0x4B450102, 0x4B450103), "N below the 256-thread block; two-polynomial body sum; three rows per level"),
    Case(O.TOY_K1, 1, (0x4B450201, 0x4B450202, 0x4B450203), "N equal to the block; two levels"),
    Case(_shape("TOY_N256_K5"), 1, (0x4B450301, 0x4B450302, 0x4B450303), "six rows per level; five-term body sum; in_dim = 1280"),
    Case(_shape("TOY_N512_K2_L2"), 1, (0x4B450401, 0x4B450402, 0x4B450403), "strided coefficient loop; k = 2 with L = 2"),
    Case(_shape("TOY_N512_K3"), 1, (0x4B450501, 0x4B450502, 0x4B450504), "k = 3"),
    Case(_shape("TOY_N16384_L3"), 1, (0x4B450602, 0x4B450605, 0x4B450606),
         "three levels, base 2^11, shifts 53 / 42 / 31; a long sequential draw per row", per_bit=0),
    Case(dataclasses.replace(O.TOY_K1, n=15, name="TOY_K1_ODD_N15"), 1, (0x4B450701, 0x4B450702, 0x4B450703),
         "keyswitch-key rows of an even number of words; small key of odd length"),
    Case(O.TOY_MULTI_BIT_N256, 2, (0x4B450801, 0x4B450802, 0x4B450803), "GGSW plaintexts are products of key bits: 32 GGSWs"),
    Case(O.TOY_MULTI_BIT_N256_G3, 3, (0x4B450901, 0x4B450902, 0x4B450906), "products of three key bits: 40 GGSWs, n = 15"),
    Case(O.TOY_MULTI_BIT_N128_K2, 2, (0x4B450A01, 0x4B450A02, 0x4B450A03), "multi-bit with k = 2"),
    Case(O.TOY_MULTI_BIT_N512_K3_G3, 3, (0x4B450B01, 0x4B450B03, 0x4B450B04), "multi-bit with k = 3, three key bits per group"),
    Case(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 1, (0x4B450C01,),
         "real dimensions: sample counts that make the bounds tight (keyswitch key M = 10,240, 24 GGSWs M = 98,304)", per_bit=11),
]
BY_NAME = {c.name: c for c in CASES}


def fhestr_params(case):
    import fhestr
    p = case.params
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name, case.grouping)


def ggsw_indices(case, bits):
    """The GGSWs whose residuals are computed: all, or the first, the last and up to per_bit more of each plaintext bit."""
    if case.per_bit is None:
        return np.arange(bits.size)
    pick = {0, bits.size - 1}
    for v in (0, 1):
        pick.update(int(i) for i in np.flatnonzero(bits == v)[:case.per_bit])
    idx = np.array(sorted(pick))
    assert 2 * idx.size >= bits.size or bits.size > 64               # a toy key: never fewer than half of its rows
    return idx


_HOST = {}


def host_keys(case, seed):
    """(client key, glwe_sk, small_sk, GGSW bits from the definition, bsk, ksk) of the host client for this seed (cached)."""
    import fhestr
    key = (case.name, seed)
    if key not in _HOST:
        ck = fhestr.ClientKey(fhestr_params(case), seed)
        g, s = ck.secret_keys()
        bsk, ksk = ck.gen_server_keys(8)
        for a in (g, s, bsk, ksk):
            a.setflags(write=False)
        _HOST[key] = (ck, g, s, X.ggsw_bits(case.params, s, case.grouping), bsk, ksk)
    return _HOST[key]


def check_inputs(case, keys_per_seed):
    """What the fixed secret keys have to provide, asserted on the inputs.  Every key: binary, both plaintext bits among the
    GGSWs whose residuals are computed, both values in each secret key.  Multi-bit: every selector value carries the bit 1 in
    some group of some seed's key -- one key cannot do that alone when it has fewer than 2^G groups (n / G = 5 and 3 for the
    two G = 3 shapes), which is one reason every shape has three seeds."""
    hit = set()
    for _, g, s, bits, _, _ in keys_per_seed:
        assert set(np.unique(g)) == {0, 1} and set(np.unique(s)) == {0, 1}, case.name
        assert set(np.unique(bits[ggsw_indices(case, bits)])) == {0, 1}, case.name
        if case.grouping > 1:
            per_group = bits.reshape(-1, 1 << case.grouping)
            assert (per_group.sum(axis=1) == 1).all()
            hit.update(int(v) for v in per_group.argmax(axis=1))
    if case.grouping > 1:
        assert hit == set(range(1 << case.grouping)), f"{case.name}: selectors with bit 1: {sorted(hit)}"


def residuals(case, g, s, bits, bsk, ksk):
    """(ksk residuals, bsk residuals) from the definition, the latter on ggsw_indices."""
    p = case.params
    return X.ksk_noise(p, ksk, g, s), X.bsk_noise(p, bsk, g, bits, ggsw_indices(case, bits))


def check_keys_from_definition(case, keys_per_seed, label):
    """(b) of every test: the residuals of each seed's keys pass distinct_streams, and pooled over the seeds normal_checks.
    keys_per_seed: (glwe_sk, small_sk, bits, bsk, ksk) per seed.  Returns the two variance ratios."""
    p = case.params
    kres, bres = [], []
    for g, s, bits, bsk, ksk in keys_per_seed:
        kr, br = residuals(case, g, s, bits, bsk, ksk)
        X.distinct_streams(ksk, bsk, p, case.n_ggsw, kr, br)
        kres.append(kr.reshape(-1))
        bres.append(br.reshape(-1))
    kres, bres = np.concatenate(kres), np.concatenate(bres)
    ratios = (X.variance_ratio(kres, p.lwe_std), X.variance_ratio(bres, p.glwe_std))
    print(f"{label} {case.name}: var/sigma^2 ksk {ratios[0]:.4f} (M = {kres.size}), bsk {ratios[1]:.4f} (M = {bres.size})")
    X.normal_checks(kres, p.lwe_std, f"{case.name} keyswitch key ({label})")
    X.normal_checks(bres, p.glwe_std, f"{case.name} bootstrapping key ({label})")
    return ratios
