"""Public-key clients on the CPU: compact public keys, compact ciphertext lists, their expansion on the host and their
byte forms (csrc/compact_pk.cpp, csrc/wire_format.cpp), against a numpy restatement of the reference's algorithms
(tests/compact_ref.py; the oracle has no compact code).  The device side is tests/test_gpu_compact_pk.py."""
import dataclasses
import struct

import numpy as np
import pytest

import compact_ref as R
import oracle as O
from conftest import to_fhestr_params

P22, P21, P11 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, O.PARAM_MESSAGE_2_CARRY_1_KS_PBS, O.PARAM_MESSAGE_1_CARRY_1_KS_PBS


def _f():
    import fhestr
    return fhestr


def _w():
    from fhestr import wire
    return wire


def _rand(rng, n):
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


def test_conv_known_answer():
    """The doctest of slice_semi_reverse_negacyclic_convolution (slice_algorithms.rs:613-620), through the library's
    convolution and through the restatement."""
    want = np.array([-17, 5, 32], dtype=np.int64).astype(np.uint64)
    assert np.array_equal(_f().compact_conv([1, 2, 3], [4, 5, 6]), want)
    assert np.array_equal(R.conv([1, 2, 3], [4, 5, 6]), want)


@pytest.mark.parametrize("n", [4, 8, 256, 2048])
@pytest.mark.parametrize("threads", [1, 5])
def test_conv_against_the_restatement(n, threads):
    """Binary right-hand sides (what key generation and encryption use) and arbitrary ones, several threads."""
    rng = np.random.default_rng(100 + n)
    lhs = _rand(rng, n)
    for rhs in (rng.integers(0, 2, size=n, dtype=np.uint64), _rand(rng, n) if n <= 256 else rng.integers(0, 2, size=n, dtype=np.uint64),
                np.zeros(n, dtype=np.uint64), np.ones(n, dtype=np.uint64)):
        assert np.array_equal(_f().compact_conv(lhs, rhs, threads), R.conv(lhs, rhs))


@pytest.mark.parametrize("params", [O.TOY_K1, O.TOY_K2], ids=lambda p: p.name)
@pytest.mark.parametrize("count", [1, 255, 256, 257, 700])
def test_expand_host_equals_the_restatement(params, count):
    """Random containers, word for word: ragged last bin, three bins."""
    P = to_fhestr_params(params)
    n = P.k * P.N
    assert n == 256
    clist = _rand(np.random.default_rng(count), _f().compact_list_len(P, count))
    assert clist.size == R.list_len(n, count) == -(-count // n) * n + count
    got = _f().expand_compact_host(P, clist, count)
    assert got.shape == (count, n + 1)
    assert np.array_equal(got, R.expand(n, clist, count))
    assert np.array_equal(_f().expand_compact_host(n, clist, count), got)


def test_expand_host_refuses_bad_shapes():
    f = _f()
    with pytest.raises(f.FheError, match="power-of-two"):
        f.expand_compact_host(1536, np.zeros(1537, dtype=np.uint64), 1)
    with pytest.raises(f.FheError, match="do not hold"):
        f.expand_compact_host(256, np.zeros(256 + 2, dtype=np.uint64), 1)


@pytest.mark.parametrize("params,count", [(O.TOY_K1, 700), (O.TOY_K2, 300), (P22, 2049), (P21, 100)], ids=lambda v: getattr(v, "name", str(v)))
def test_public_key_round_trip(params, count):
    """ClientKey -> public key -> encrypt -> host expansion -> ClientKey.decrypt gives m mod msg_mod; the same seed gives
    the same bytes whatever the thread count, another seed another list."""
    f = _f()
    P = to_fhestr_params(params)
    ck = f.ClientKey(P, 0xC0FFEE)
    pk = ck.compact_public_key(0xBEEF)
    assert pk.words.size == f.compact_pk_len(P) == 2 * P.k * P.N
    msgs = np.random.default_rng(7).integers(0, 4 * P.msg_mod * P.carry_mod, size=count, dtype=np.uint64)
    clist = pk.encrypt(msgs, 0x5EED, threads=3)
    assert clist.size == f.compact_list_len(P, count)
    cts = f.expand_compact_host(P, clist, count)
    assert np.array_equal(ck.decrypt(cts), (msgs % P.msg_mod).astype(np.int64))
    assert np.array_equal(pk.encrypt(msgs, 0x5EED, threads=1), clist)
    assert np.array_equal(ck.compact_public_key(0xBEEF).words, pk.words)
    other = pk.encrypt(msgs, 0x5EEE)
    assert not np.array_equal(other, clist)
    assert np.array_equal(ck.decrypt(f.expand_compact_host(P, other, count)), (msgs % P.msg_mod).astype(np.int64))
    assert not np.array_equal(ck.compact_public_key(0xBEF0).words, pk.words)


def test_encrypt_string_is_the_block_list():
    f = _f()
    P = to_fhestr_params(O.TOY_K1)
    ck = f.ClientKey(P, 3)
    pk = ck.compact_public_key(4)
    clist = pk.encrypt_string(b"Zama", 6, 5)
    assert np.array_equal(clist, pk.encrypt(f.string_to_blocks(P, b"Zama", 6), 5))
    blocks = ck.decrypt(f.expand_compact_host(P, clist, 6 * f.blocks_per_char(P)))
    assert f.blocks_to_string(P, blocks) == b"Zama"


@pytest.mark.parametrize("params", [O.TOY_K1, P22, P21], ids=lambda p: p.name)
def test_public_key_is_a_valid_key(params):
    """b - conv(a, s), with the restatement's convolution and the client's secret key, is the key's noise: every entry
    below eight standard deviations (2,048 draws: 8 sigma is never reached by a correct sampler)."""
    f = _f()
    P = to_fhestr_params(params)
    n = P.k * P.N
    ck = f.ClientKey(P, 0xA11CE)
    pk = ck.compact_public_key(0xB0B).words
    s, _ = ck.secret_keys()
    e = (pk[n:] - R.conv(pk[:n], s)).astype(np.int64)
    bound = 8 * P.glwe_std * 2.0**64
    assert np.abs(e).max() < bound, (np.abs(e).max(), bound)
    assert np.abs(e).max() > 0            # ... and it is there


def test_noise_of_the_whole_route_p22():
    """PARAM_MESSAGE_2_CARRY_2 dimensions, 32 independent (client seed, key seed, encryption seed) triples, one full bin of
    2,048 ciphertexts each: the root mean square (not mean-subtracted) of phase - delta * m over all 65,536 ciphertexts,
    divided by glwe_std * 2^64 * sqrt(1 + n/2 + |s|^2) averaged the same way, lies in [0.85, 1.15].  The phase error is
    conv(e, r)[c] + e2[c] - conv(e1, s)[c]: variance sigma^2 (1 + |r|^2 + |s|^2).  The errors of one bin are correlated
    (binary r and s have mean 1/2), so one bin scatters by 17 %; over 32 bins the ratio has a standard deviation of
    about 0.036 (simulated with the reference formulas), the band is four of those.  Leaving out e1 or the key's e
    gives 0.70."""
    f = _f()
    P = to_fhestr_params(P22)
    n = P.k * P.N
    rng = np.random.default_rng(2048)
    sq_sum, model_sum = 0.0, 0.0
    for t in range(32):
        ck = f.ClientKey(P, 0x10000 + t)
        pk = ck.compact_public_key(0x20000 + t)
        msgs = rng.integers(0, P.msg_mod, size=n, dtype=np.uint64)
        cts = f.expand_compact_host(P, pk.encrypt(msgs, 0x30000 + t), n)
        s, _ = ck.secret_keys()
        with np.errstate(over="ignore"):
            err = (R.phases(cts, s) - np.uint64(P.delta) * msgs).astype(np.int64).astype(np.float64)
        sq_sum += float(np.mean(err**2))
        model_sum += (P.glwe_std * 2.0**64) ** 2 * (1 + n / 2 + float(s.sum()))
    ratio = (sq_sum / model_sum) ** 0.5
    print(f"compact public-key route, P22, 32 bins: rms error / model = {ratio:.4f}")
    assert 0.85 <= ratio <= 1.15, ratio


@pytest.mark.parametrize("params", [P11, dataclasses.replace(O.TOY_K1, k=5, N=256, name="K5_N256")], ids=lambda p: p.name)
def test_dimensions_that_are_not_a_power_of_two_are_refused(params):
    """k = 3, N = 512 and k = 5, N = 256: the reference's CompactPublicKey::try_new returns None (compact.rs:65)."""
    f = _f()
    P = to_fhestr_params(params)
    assert f.compact_pk_len(P) == 0 and f.compact_list_len(P, 10) == 0
    ck = f.ClientKey(P, 1)
    with pytest.raises(f.FheError, match="power-of-two"):
        ck.compact_public_key(2)
    # the C entry points themselves, not only the Python guards
    import ctypes as C
    sb = (C.c_uint8 * 32)()
    buf = np.zeros(4 * P.k * P.N, dtype=np.uint64)
    assert f.lib().fhe_client_gen_compact_public_key(ck._h, sb, buf.ctypes.data_as(C.c_void_p)) != 0
    assert "power-of-two" in f.lib().fhe_last_error().decode()
    assert f.lib().fhe_compact_pk_encrypt(C.byref(P.c()), buf.ctypes.data_as(C.c_void_p), sb, buf.ctypes.data_as(C.c_void_p), 1,
                                          buf.ctypes.data_as(C.c_void_p), 1) != 0
    assert "power-of-two" in f.lib().fhe_last_error().decode()
    assert f.lib().fhe_compact_expand_host(P.k * P.N, buf.ctypes.data_as(C.c_void_p), 1, buf.ctypes.data_as(C.c_void_p)) != 0
    with pytest.raises(f.FheError, match="power-of-two"):
        _w().read_compact_public_key(P, b"\0" * 64)


# ---- byte forms ------------------------------------------------------------------------------------------------------

_MODULUS = struct.pack("<QQQ", 0, 0, 64)     # CiphertextModulus<u64>: u128 0 (native), scalar_bits 64


def _toy_list(count):
    f = _f()
    P = to_fhestr_params(O.TOY_K1)
    ck = f.ClientKey(P, 21)
    pk = ck.compact_public_key(22)
    msgs = np.arange(count, dtype=np.uint64) % P.msg_mod
    return P, ck, pk, msgs, pk.encrypt(msgs, 23)


def test_compact_list_layouts_by_hand():
    """bincode: Vec<u64> = u64 length + words; usize newtypes = u64; struct fields in declaration order; unit enum
    variant = u32 index.  LweCompactCiphertextList { data, lwe_size, lwe_ciphertext_count, ciphertext_modulus };
    shortint CompactCiphertextList { ct_list, degree, message_modulus, carry_modulus, pbs_order, noise_level };
    integer CompactCiphertextList { ct_list, num_blocks_per_integer }."""
    w = _w()
    P, _, _, _, clist = _toy_list(3)
    assert clist.size == 256 + 3
    core = struct.pack("<Q", 259) + clist.astype("<u8").tobytes() + struct.pack("<QQ", 257, 3) + _MODULUS
    assert w.write_compact_list(P, clist, 3) == core
    meta = w.ShortintMeta(degree=3, noise_level=1, message_modulus=4, carry_modulus=4, pbs_order=0)
    assert w.compact_meta(P) == meta
    shortint = core + struct.pack("<QQQ", 3, 4, 4) + struct.pack("<I", 0) + struct.pack("<Q", 1)
    assert w.write_shortint_compact_list(P, clist, 3) == shortint
    odd = w.ShortintMeta(degree=2, noise_level=7, message_modulus=4, carry_modulus=4, pbs_order=1)
    assert w.write_shortint_compact_list(P, clist, 3, odd) == core + struct.pack("<QQQIQ", 2, 4, 4, 1, 7)
    assert w.write_shortint_compact_list(P, clist, 3, num_blocks_per_integer=3) == shortint + struct.pack("<Q", 3)


def test_compact_public_key_layout_by_hand():
    """LweCompactPublicKey { glwe_ciphertext: GlweCiphertext { data, polynomial_size, ciphertext_modulus } }."""
    w = _w()
    P, _, pk, _, _ = _toy_list(1)
    data = w.write_compact_public_key(P, pk)
    assert data == struct.pack("<Q", 512) + pk.words.astype("<u8").tobytes() + struct.pack("<Q", 256) + _MODULUS
    assert np.array_equal(w.read_compact_public_key(P, data).words, pk.words)


@pytest.mark.parametrize("count", [1, 256, 300])
def test_compact_wire_round_trips(count):
    f, w = _f(), _w()
    P, ck, pk, msgs, clist = _toy_list(count)
    got, n, used = w.read_compact_list(P, w.write_compact_list(P, clist, count) + b"tail")
    assert np.array_equal(got, clist) and n == count and used == 8 + 8 * clist.size + 16 + 24
    data = w.write_shortint_compact_list(P, clist, count)
    got, n, meta, blocks, used = w.read_shortint_compact_list(P, data)
    assert np.array_equal(got, clist) and n == count and meta == w.compact_meta(P) and blocks == 0 and used == len(data)
    if count % 4 == 0:
        data = w.write_shortint_compact_list(P, clist, count, num_blocks_per_integer=4)
        got, n, meta, blocks, used = w.read_shortint_compact_list(P, data, integer=True)
        assert np.array_equal(got, clist) and n == count and blocks == 4 and used == len(data)
    # a list that came over the wire decrypts; a key that came over the wire encrypts
    assert np.array_equal(ck.decrypt(f.expand_compact_host(P, got, n)), msgs.astype(np.int64))
    pk2 = w.read_compact_public_key(P, w.write_compact_public_key(P, pk))
    assert np.array_equal(pk2.encrypt(msgs, 23), clist)


def test_compact_readers_refuse():
    f, w = _f(), _w()
    P, _, pk, _, clist = _toy_list(3)
    core = w.write_compact_list(P, clist, 3)
    shortint = w.write_shortint_compact_list(P, clist, 3)
    integer = w.write_shortint_compact_list(P, clist, 3, num_blocks_per_integer=3)
    key = w.write_compact_public_key(P, pk)
    # truncated anywhere: never read past in_len
    for data, read in ((core, lambda d: w.read_compact_list(P, d)), (shortint, lambda d: w.read_shortint_compact_list(P, d)),
                       (integer, lambda d: w.read_shortint_compact_list(P, d, integer=True)), (key, lambda d: w.read_compact_public_key(P, d))):
        for cut in (0, 7, 8, 100, len(data) - 17, len(data) - 1):
            with pytest.raises(f.FheError, match="truncated"):
                read(data[:cut])
    # a length field that promises more than the input / the destination holds
    huge = struct.pack("<Q", 2**61) + core[8:]
    with pytest.raises(f.FheError, match="longer than the destination|truncated"):
        w.read_compact_list(P, huge)
    with pytest.raises(f.FheError, match="longer than the destination|truncated"):
        w.read_compact_public_key(P, struct.pack("<Q", 2**61) + key[8:])
    with pytest.raises(f.FheError, match="more than the destination holds|longer than the destination"):
        w.read_compact_list(P, core, max_count=2)
    # container length against the count (lwe_compact_ciphertext_list_size)
    words = clist.astype("<u8").tobytes()
    for bad_count in (2, 4, 0, 257):
        lying = struct.pack("<Q", 259) + words + struct.pack("<QQ", 257, bad_count) + _MODULUS
        with pytest.raises(f.FheError, match="does not hold"):
            w.read_compact_list(P, lying)
    short = struct.pack("<Q", 258) + words[:-8] + struct.pack("<QQ", 257, 3) + _MODULUS
    with pytest.raises(f.FheError, match="does not hold"):
        w.read_compact_list(P, short)
    # dimensions and moduli against the parameter set
    with pytest.raises(f.FheError, match="lwe_size"):
        w.read_compact_list(P, struct.pack("<Q", 259) + words + struct.pack("<QQ", 129, 3) + _MODULUS)
    with pytest.raises(f.FheError, match="64 bits"):
        w.read_compact_list(P, core[:-8] + struct.pack("<Q", 32))
    with pytest.raises(f.FheError, match="native modulus"):
        w.read_compact_list(P, core[:-24] + struct.pack("<QQQ", 1 << 32, 0, 64))
    with pytest.raises(f.FheError, match="parameter set"):
        w.read_shortint_compact_list(P, core + struct.pack("<QQQIQ", 3, 2, 4, 0, 1))
    with pytest.raises(f.FheError, match="PBSOrder"):
        w.read_shortint_compact_list(P, core + struct.pack("<QQQIQ", 3, 4, 4, 2, 1))
    with pytest.raises(f.FheError, match="multiple"):
        w.read_shortint_compact_list(P, shortint + struct.pack("<Q", 2), integer=True)
    with pytest.raises(f.FheError, match="multiple"):
        w.read_shortint_compact_list(P, shortint + struct.pack("<Q", 0), integer=True)
    with pytest.raises(f.FheError, match="parameter set"):
        w.read_compact_public_key(P, struct.pack("<Q", 512) + pk.words.tobytes() + struct.pack("<Q", 512) + _MODULUS)
    other = to_fhestr_params(O.TOY_N8192)
    with pytest.raises(f.FheError):
        w.read_compact_public_key(other, key)
    with pytest.raises(f.FheError, match="lwe_size"):
        w.read_compact_list(other, core)
    with pytest.raises(f.FheError, match="multiple"):
        w.write_shortint_compact_list(P, clist, 3, num_blocks_per_integer=2)
