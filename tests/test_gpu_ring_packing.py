"""Ring packing on the device (csrc/ring_packing_kernels.hip.h, fhe::Packing in csrc/packing_dev.hip) against the host
reference fhe_ring_pack_host, which tests/test_ring_packing.py pins to the definition in Python integers.

  test_device_equals_host         the packed GLWEs word for word: uniform key words and LWEs (the comparison needs no valid
                                  key), every shape family up to PARAM_MESSAGE_4_CARRY_4's N = 32768 -- the full-LDS
                                  transform, 42 automorphism keyswitches for three blocks; the info record against the cost formula
  test_device_transform           the device transform alone against the host's, the all-extreme input included
  test_noise_on_the_device        4,096 packed coefficients of TOY_K1 against the model, in the band of the host measurement
  test_p22_*                      packed=True with only a ring key loaded; a refresh-grade pair goes back into contains; the
                                  refresh gate admits and refuses where fhe_ring_packing_noise / fhe_ring_narrow_noise say
  test_p44_*                      PARAM_MESSAGE_4_CARRY_4, which the matrix route refuses: three packed blocks decrypt, full, at
                                  20 bits, and -- trivially encrypted -- at 13 bits"""
import math

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
import exact_ring_packing as X
from test_ring_packing import NOISE_BAND, NOISE_MEASURED

pytestmark = pytest.mark.gpu

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
P44 = O.PARAM_MESSAGE_4_CARRY_4_KS_PBS
K3_N512 = next(p for p in O.TOY_SHAPES if p.name == "TOY_N512_K3")
K2_N1024 = next(p for p in O.TOY_SHAPES if p.name == "TOY_N1024_K2")

_ENGINES = {}


def _engine(p):
    """An engine without server keys, one per shape."""
    import fhestr
    if p.name not in _ENGINES:
        _ENGINES[p.name] = fhestr.Engine(to_fhestr_params(p), 0)
    return _ENGINES[p.name]


WORD_CASES = [(O.TOY_K1, [1, 3, 256, 257]), (K3_N512, [5]), (K2_N1024, [33]), (P22, [33, 1024]), (O.TOY_N8192, [3]), (P44, [3])]


@pytest.mark.parametrize("p,counts", WORD_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_device_equals_host(p, counts):
    import fhestr
    P = to_fhestr_params(p)
    pair = fhestr.ring_packing_default_params(P)
    rng = np.random.default_rng([p.N, p.k])
    key = X.edge_key(p, pair, rng)
    eng = _engine(p)
    eng.load_ring_packing_key(pair, key)
    for count in counts:
        cts = rng.integers(0, 2**64, size=(count, P.big_size), dtype=np.uint64)
        cts[0, :4] = [0, 2**64 - 1, 2**63, 2**63 - 1]
        want = fhestr.ring_pack_host(P, pair, key, cts)
        got = eng.pack(cts)
        assert got.shape == want.shape == (-(-count // p.N), p.k + 1, p.N)
        bad = np.argwhere(got != want)
        assert not len(bad), f"count {count}: {len(bad)} of {want.size} words differ; first (glwe, polynomial, coefficient) {bad[:8].tolist()}"
        info = eng.ring_pack_info()
        assert info["ran"] and info["levels"] == p.N.bit_length() - 1
        assert info["keyswitches"] == X.keyswitch_count(p.N, count) == fhestr.ring_pack_keyswitches(P, count)
        assert info["launches"] >= 1 + 3 * info["levels"] and (info["launches"] - 1) % 3 == 0
        assert count * (p.k + 1) * p.N * 8 <= info["scratch_bytes"] <= (2 << 30) + (256 << 20)
    if p is P44:
        assert info["keyswitches"] == 42


@pytest.mark.parametrize("N", [64, 2048, 32768])
def test_device_transform(N):
    import fhestr
    eng = _engine(O.TOY_K1)
    a = np.random.default_rng(N).integers(0, X.P, size=(4, N), dtype=np.uint32)
    a[1] = X.P - 64                     # every digit -2^(b-1) at b = 7
    a[2] = X.P - 128                    # every plane word -128
    a[3, :2] = [0, X.P - 1]
    fwd = fhestr.ring_ntt_host(a)
    assert np.array_equal(eng.ring_ntt(a), fwd)
    assert np.array_equal(eng.ring_ntt(fwd, inverse=True), a)
    # the all-extreme product through the device transforms: 7 terms at N = 32768 sit at 0.875 of P / 2
    terms = 7 if N == 32768 else 2
    prod = (fwd[1].astype(object) * fwd[2].astype(object) * terms) % X.P
    back = eng.ring_ntt(np.array([prod], dtype=np.uint32), inverse=True)[0].astype(np.int64)
    lifted = np.where(back > X.P // 2, back - X.P, back)
    assert np.array_equal(lifted, 64 * 128 * terms * (2 * np.arange(N, dtype=np.int64) + 2 - N))


def _phase_errors(P, glwe_sk, glwes, msgs):
    """(phase - message delta) / 2^64 of every packed coefficient, signed: [G, N]."""
    N, k = P.N, P.k
    delta = np.uint64(2**63 // (P.msg_mod * P.carry_mod))
    glwes = np.asarray(glwes, dtype=np.uint64).reshape(-1, k + 1, N)
    ph = glwes[:, k, :].copy()
    with np.errstate(over="ignore"):
        for q in range(k):
            s = glwe_sk[q * N:(q + 1) * N]
            m = np.zeros((N, N), dtype=np.uint64)
            for t in np.nonzero(s)[0]:
                idx = np.arange(N)
                m[idx[:N - t], idx[:N - t] + t] += np.uint64(1)
                m[idx[N - t:], idx[N - t:] + t - N] -= np.uint64(1)
            ph -= glwes[:, q, :] @ m
        ph -= np.asarray(msgs, dtype=np.uint64).reshape(ph.shape) * delta
    return ph.astype(np.int64).astype(np.float64) / 2.0**64


def test_noise_on_the_device():
    """TOY_K1 (N = 256) under the pair (5, 3), whose rounding term rules as on the named sets: 16 GLWEs of fresh encryptions
    of 0, packed on the device.  Band: the two host measurements of tests/test_ring_packing.py, each with the 3 sigma of
    4,096 samples."""
    import fhestr
    p, pair = O.TOY_K1, (5, 3)
    P = to_fhestr_params(p)
    ck = fhestr.ClientKey(P, 0x5EED0F00)
    pair, key = ck.gen_ring_packing_key(pair, seed=13)
    eng = _engine(p)
    eng.load_ring_packing_key(pair, key)
    count = 16 * p.N
    glwes = eng.pack(ck.encrypt(np.zeros(count, dtype=np.int64)))
    err = _phase_errors(P, ck.secret_keys()[0], glwes, np.zeros(count, dtype=np.int64))
    ratio = float(np.mean(err**2)) / (X.variance(p, pair) + p.glwe_std**2)
    print(f"ring packing noise on the device {p.name} {pair}: measured / modelled variance {ratio:.3f}")
    assert min(NOISE_MEASURED.values()) * (1 - NOISE_BAND) <= ratio <= max(NOISE_MEASURED.values()) * (1 + NOISE_BAND)
    ck.close()


class _Rig:
    """PARAM_MESSAGE_2_CARRY_2 with server keys generated on the device and only a ring packing key loaded."""

    def __init__(self):
        import fhestr
        self.P = to_fhestr_params(P22)
        self.ck = fhestr.ClientKey(self.P, 0x5EED1000)
        self.eng = fhestr.Engine(self.P, 0)
        glwe_sk, small_sk = self.ck.secret_keys()
        self.eng.generate_keys(glwe_sk, small_sk, 0x5EED1001)
        self.pair = None

    def ring_key(self, pair):
        if pair != self.pair:
            self.pair, key = self.ck.gen_ring_packing_key(pair, seed=0x5EED1002)
            self.eng.load_ring_packing_key(self.pair, key)
        return self.pair


_RIG = []


def _rig():
    if not _RIG:
        _RIG.append(_Rig())
    return _RIG[0]


REFRESH_PAIR = (12, 3)          # 1.00005 nominal variances against a budget of 138; the default (12, 2) carries 752


def test_p22_packed_result_with_only_a_ring_key():
    import fhestr
    rig = _rig()
    assert rig.ring_key(fhestr.ring_packing_default_params(rig.P)) == (12, 2)
    P, eng, ck = rig.P, rig.eng, rig.ck
    ops = fhestr.FheStringOps(eng)
    cap = 8
    n_blocks = cap * ops.bpc
    up = ops.to_upper(ck.encrypt(fhestr.string_to_blocks(P, b"a Fox", cap)), packed=True)
    assert isinstance(up, fhestr.PackedString) and (up.count, up.capacity) == (n_blocks, cap) and up.shape == (1, P.k + 1, P.N)
    assert eng.ring_pack_info()["keyswitches"] == X.keyswitch_count(P.N, n_blocks)
    assert not eng.packing_info()["ran"]                       # the matrix route never ran
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(up, n_blocks)) == b"A FOX"
    ops.close()


def test_p22_packed_string_goes_back_in():
    import fhestr
    rig = _rig()
    pair = rig.ring_key(REFRESH_PAIR)
    nominal, budget = fhestr.ring_packing_noise(rig.P, pair)
    assert nominal <= budget
    P, eng, ck = rig.P, rig.eng, rig.ck
    ops = fhestr.FheStringOps(eng)
    cap = 8
    enc = lambda t, c=cap: ck.encrypt(fhestr.string_to_blocks(P, t, c))
    up = ops.to_upper(enc(b"a Fox"), packed=True)
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(up, up.count)) == b"A FOX"
    for pat in (b"FOX", b"Fox"):
        got = ops.contains(up, enc(pat, 4))                    # the packed result straight back in
        assert eng.unpack_info()["refreshed"]
        assert ck.decrypt(got.reshape(1, -1))[0] == int(pat in b"A FOX")
    narrow = ops.to_lower(up, packed=fhestr.Narrow())          # the operand-grade default width of the ring pair
    assert isinstance(narrow, fhestr.NarrowString) and narrow.bits == fhestr.ring_narrow_default_bits(P, pair)
    assert fhestr.blocks_to_string(P, ck.decrypt_narrow(narrow)) == b"a fox"
    assert ck.decrypt(ops.contains(narrow, enc(b"fox", 4)).reshape(1, -1))[0] == 1
    ops.close()


def test_p22_refresh_gate_follows_the_ring_model():
    import fhestr
    rig = _rig()
    P, eng, ck = rig.P, rig.eng, rig.ck
    msgs = np.arange(8) % 16
    for pair in ((12, 2), REFRESH_PAIR):
        rig.ring_key(pair)
        nominal, budget = fhestr.ring_packing_noise(P, pair)
        glwes = eng.pack(ck.encrypt(msgs))
        assert np.array_equal(ck.decrypt(eng.unpack(glwes, 8, refresh=False)), msgs)      # raw extraction needs no judgement
        if nominal > budget:
            before = eng.unpack_info()
            with pytest.raises(fhestr.FheError, match="refresh refused.*ring packing pair"):
                eng.unpack(glwes, 8, refresh=True)
            assert eng.unpack_info() == before
        else:
            assert np.array_equal(ck.decrypt(eng.unpack(glwes, 8, refresh=True)), msgs)
        for bits in (8, 13, 20):
            v = fhestr.ring_narrow_noise(P, pair, bits)
            narrow = eng.narrow(glwes, held=8, bits=bits)
            if v[0] > v[1]:
                with pytest.raises(fhestr.FheError, match="refresh refused"):
                    eng.unpack_narrow(narrow, refresh=True)
            else:
                assert np.array_equal(ck.decrypt(eng.unpack_narrow(narrow, refresh=True)), msgs)
    assert (fhestr.ring_packing_noise(P, (12, 2))[0] > budget) and (fhestr.ring_packing_noise(P, REFRESH_PAIR)[0] <= budget)


_P44, _P44_KEY = [], []


def _p44():
    """PARAM_MESSAGE_4_CARRY_4 with its default ring key (7, 5), 39 MB; no server keys.  Three blocks, packed once."""
    import fhestr
    if not _P44:
        P = to_fhestr_params(P44)
        ck = fhestr.ClientKey(P, 0x5EED1100)
        pair, key = ck.gen_ring_packing_key(seed=0x5EED1101)
        assert pair == (7, 5) and key.nbytes == 39321600
        with pytest.raises(fhestr.FheError, match="unsupported parameter set"):
            fhestr.packing_default_params(P)                    # the matrix route still refuses this set
        eng = _engine(P44)
        eng.load_ring_packing_key(pair, key)
        _P44_KEY.append(key)
        msgs = np.array([5, 200, 255])
        _P44.append((P, ck, eng, msgs, eng.pack(ck.encrypt(msgs))))
    return _P44[0]


def test_p44_three_blocks_decrypt_packed():
    P, ck, eng, msgs, glwes = _p44()
    assert glwes.shape == (1, 2, 32768)
    assert np.array_equal(ck.decrypt_packed(glwes, 3), msgs)


def test_p44_three_blocks_decrypt_narrow_13():
    """Three trivially encrypted blocks (zero mask, body m delta), packed on the device, narrowed to 13 bits, decrypted.  A
    trivial LWE has a zero leaf mask, every digit of its automorphism keyswitches is 0, so the packed GLWE is (0, B) with
    B[j] = N * ((m_j delta + N/2) >> log2 N): narrowing rounds only the body, by at most 2^-14 against delta / 2 = 2^-10, and
    the blocks decode whatever the key.  Fresh encryptions do NOT decode at 13 bits on this set -- the mask's rounding against
    kN/2 = 16,384 key bits has standard deviation 2^-7.8 (fhe_ring_narrow_noise: log2 of the failure probability -0.27 at 13
    bits, -37 at 18, -419 at 20; measured: [5, 200, 255] came back as [6, 200, 255]) -- which the assertions on the model
    below pin, and test_p44_three_blocks_decrypt_narrow_20 is the fresh case at a width the model admits."""
    import fhestr
    P, ck, eng, msgs, _ = _p44()
    trivial = np.zeros((3, P.big_size), dtype=np.uint64)
    trivial[:, -1] = msgs.astype(np.uint64) * np.uint64(2**63 // (P.msg_mod * P.carry_mod))
    glwes = eng.pack(trivial)
    assert np.array_equal(glwes, fhestr.ring_pack_host(P, (7, 5), _P44_KEY[0], trivial))
    assert not glwes[0, 0].any() and not glwes[0, 1, 3:].any()       # no mask, and nothing beyond the three blocks
    assert np.array_equal(ck.decrypt_packed(glwes, 3), msgs)
    narrow = eng.narrow(glwes, held=3, bits=13)
    assert isinstance(narrow, fhestr.NarrowString) and narrow.bits == 13
    assert np.array_equal(narrow, fhestr.glwe_narrow_host(P, glwes, 3, 13).reshape(narrow.shape))
    assert np.array_equal(ck.decrypt_narrow(narrow), msgs)
    # what the model says about PBS outputs and fresh encryptions at this width: not client-grade, let alone operand-grade
    nominal, budget, log2_pfail = fhestr.ring_narrow_noise(P, (7, 5), 13)
    assert nominal > budget and log2_pfail > -1


def test_p44_three_blocks_decrypt_narrow_20():
    import fhestr
    P, ck, eng, msgs, glwes = _p44()
    assert fhestr.ring_narrow_noise(P, (7, 5), 20)[2] < -40
    narrow = eng.narrow(glwes, held=3, bits=20)
    assert np.array_equal(narrow, fhestr.glwe_narrow_host(P, glwes, 3, 20).reshape(narrow.shape))
    assert np.array_equal(ck.decrypt_narrow(narrow), msgs)
