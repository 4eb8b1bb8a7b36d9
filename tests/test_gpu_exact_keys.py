"""Device key generation (ksk_gen_kernel, bsk_gen_kernel; csrc/keygen_kernels.hip.h) at every shape of tests/key_cases.py:
(a) both exported keys equal the host client's word for word, (b) their residuals from the DEFINITION of the encryptions
(tests/exact_keys.py) are centred normal noise of the parameter set's deviation from streams that never repeat, (c) the
installed key is the exported one: a lookup table on eight messages decrypts.  (a) alone compares a formula with its copy;
(b) alone would not notice a device that differs from the host within the noise.  The other device path that manufactures key
material, the seeded-key expansion, is compared with the host's at an odd n."""
import numpy as np
import pytest

import oracle as O
import exact_keys as X
import key_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_device_keys_equal_the_host_keys_and_follow_the_definition(case):
    import fhestr
    P = K.fhestr_params(case)
    ok, why = fhestr.params_supported(P)
    assert ok, why
    host = [K.host_keys(case, seed) for seed in case.seeds]
    K.check_inputs(case, host)
    M = P.msg_mod * P.carry_mod
    device = []
    for seed, (ck, g, s, bits, hbsk, hksk) in zip(case.seeds, host):
        eng = fhestr.Engine(P, 0)
        try:
            bsk, ksk = eng.generate_keys(g, s, seed, export=True)
            assert np.array_equal(ksk, hksk), f"{case.name} seed {seed:#x}: keyswitch key differs from the host's"       # (a)
            assert np.array_equal(bsk, hbsk), f"{case.name} seed {seed:#x}: bootstrapping key differs from the host's"
            f = lambda x: (3 * x + 1) % M
            lut, _ = eng.generate_lookup_table(f)
            msgs = np.arange(8) % M
            out = eng.apply_lookup_table(ck.encrypt(msgs), np.full(8, lut, dtype=np.uint32))                          # (c)
            assert ck.decrypt(out).tolist() == [f(int(m)) for m in msgs]
        finally:
            eng.close()
        device.append((g, s, bits, bsk, ksk))
    K.check_keys_from_definition(case, device, "device")                                                               # (b)


def test_device_keys_change_with_every_seed_word():
    """Same secret keys, seeds that differ in one of the eight 32-bit words: nine different key pairs."""
    import fhestr
    case = K.BY_NAME[O.TOY_K2.name]
    _, g, s, _, _, _ = K.host_keys(case, case.seeds[0])
    base = 0x0123456789ABCDEF_0F1E2D3C4B5A6978_1122334455667788_99AABBCCDDEEFF00
    eng = fhestr.Engine(K.fhestr_params(case), 0)
    try:
        keys = [eng.generate_keys(g, s, seed, export=True) for seed in [base] + [base ^ (1 << (32 * w)) for w in range(8)]]
    finally:
        eng.close()
    assert len({bsk.tobytes() for bsk, _ in keys}) == 9 and len({ksk.tobytes() for _, ksk in keys}) == 9
    for bsk, ksk in keys:
        X.distinct_streams(ksk, bsk, case.params)


@pytest.mark.parametrize("name", ["TOY_K1_ODD_N15", "TOY_N512_K2_L2"])
def test_seeded_keys_expand_like_the_host_at_an_odd_n(name):
    """fhe_engine_load_seeded_keys against the host decompression, word for word.  With n = 15 the two words of an AES block
    straddle two keyswitch-key rows in seeded_expand_kernel's g / mask_per_row split (every other tested shape has n even);
    N = 512, k = 2, two levels is the bootstrapping-key side with mask rows of two polynomials."""
    import fhestr
    from fhestr import wire
    P = K.fhestr_params(K.BY_NAME[name])
    rng = np.random.default_rng(0x5EED)
    kb = rng.integers(0, 1 << 63, size=wire.ksk_bodies_len(P), dtype=np.uint64)
    bb = rng.integers(0, 1 << 63, size=wire.bsk_bodies_len(P), dtype=np.uint64)
    ksk_seed, bsk_seed = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0, (1 << 127) + 9
    eng = fhestr.Engine(P, 0)
    try:
        bsk, ksk = eng.load_seeded_keys(ksk_seed, kb, bsk_seed, bb, export=True)
    finally:
        eng.close()
    assert np.array_equal(ksk, wire.decompress_keyswitch_key(P, ksk_seed, kb))
    assert np.array_equal(bsk, wire.decompress_bootstrap_key(P, bsk_seed, bb))
    assert np.array_equal(ksk.reshape(-1, P.n + 1)[:, P.n], kb)
