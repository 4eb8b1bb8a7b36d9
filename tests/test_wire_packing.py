"""Byte forms of the packing keyswitch objects (csrc/wire_format.cpp): LwePackingKeyswitchKey, GlweCiphertext and lists of
them, pinned against the bincode rules on hand-built examples (u64 lengths and usize fields, little endian; the native
modulus as u128 0 and scalar_bits 64).  Parity with a real client is unpinned, as for the other objects."""
import struct

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params

P = O.TOY_K2            # k = 2, N = 128: GLWE size 3


def _f():
    import fhestr
    return fhestr


def _w():
    from fhestr import wire
    return wire


MODULUS = struct.pack("<QQQ", 0, 0, 64)


def _vec(words):
    words = np.asarray(words, dtype="<u8").reshape(-1)
    return struct.pack("<Q", words.size) + words.tobytes()


def _key_bytes(words, base_log, level, glwe_size, poly):
    return _vec(words) + struct.pack("<QQQQ", base_log, level, glwe_size, poly) + MODULUS


def _glwe_bytes(words, poly):
    return _vec(words) + struct.pack("<Q", poly) + MODULUS


def _key(pp):
    return np.random.default_rng(pp).integers(0, 2**64, size=P.k * P.N * pp[1] * (P.k + 1) * P.N, dtype=np.uint64)


@pytest.mark.parametrize("pp", [(7, 2), (3, 5)], ids=str)
def test_packing_key_round_trip(pp):
    FP = to_fhestr_params(P)
    key = _key(pp)
    data = _w().write_packing_key(FP, pp, key)
    assert data == _key_bytes(key, pp[0], pp[1], P.k + 1, P.N)
    got_pp, got = _w().read_packing_key(FP, data)
    assert got_pp == pp and np.array_equal(got, key)
    got_pp, got = _w().read_packing_key(FP, data + b"trailing")
    assert got_pp == pp and np.array_equal(got, key)


def test_packing_key_refusals():
    FP, pp = to_fhestr_params(P), (7, 2)
    key = _key(pp)
    good = _key_bytes(key, 7, 2, P.k + 1, P.N)
    E = _f().FheError
    for cut in (0, 7, 8, 8 + 8 * key.size - 1, len(good) - 41, len(good) - 24, len(good) - 1):
        with pytest.raises(E, match="truncated"):
            _w().read_packing_key(FP, good[:cut])
    for bad in (_key_bytes(key, 7, 2, P.k + 2, P.N),            # another GLWE size
                _key_bytes(key, 7, 2, P.k + 1, 2 * P.N),        # another polynomial size
                _key_bytes(key[:-1], 7, 2, P.k + 1, P.N),       # a word short
                _key_bytes(key, 7, 1, P.k + 1, P.N)):           # the container of two levels under one
        with pytest.raises(E, match="does not match"):
            _w().read_packing_key(FP, bad)
    with pytest.raises(E, match="unsupported packing decomposition"):
        _w().read_packing_key(FP, _key_bytes(key, 8, 2, P.k + 1, P.N))
    with pytest.raises(E, match="native modulus"):
        _w().read_packing_key(FP, good[:-24] + struct.pack("<QQQ", 1 << 32, 0, 64))
    with pytest.raises(E):
        _w().write_packing_key(FP, pp, key[:-1])
    # a length field that promises more than the input holds is refused before anything is copied
    with pytest.raises(E, match="truncated"):
        _w().read_packing_key(FP, struct.pack("<Q", 1 << 60) + good[8:])


def test_glwe_round_trip_and_refusals():
    FP = to_fhestr_params(P)
    E = _f().FheError
    glwes = np.random.default_rng(5).integers(0, 2**64, size=(3, P.k + 1, P.N), dtype=np.uint64)
    one = _w().write_glwe_ciphertext(FP, glwes[0])
    assert one == _glwe_bytes(glwes[0], P.N)
    got, used = _w().read_glwe_ciphertext(FP, one + b"xx")
    assert used == len(one) and np.array_equal(got, glwes[0])
    data = _w().write_glwe_list(FP, glwes)
    assert data == struct.pack("<Q", 3) + b"".join(_glwe_bytes(g, P.N) for g in glwes)
    assert np.array_equal(_w().read_glwe_list(FP, data), glwes)
    assert _w().read_glwe_list(FP, _w().write_glwe_list(FP, glwes[:0])).shape == (0, P.k + 1, P.N)
    for cut in (0, 5, 8, len(one) + 7, len(data) - 1):
        with pytest.raises(E, match="truncated"):
            _w().read_glwe_list(FP, data[:cut])
    with pytest.raises(E, match="destination holds"):
        _w().read_glwe_list(FP, data, max_glwes=2)
    with pytest.raises(E, match="does not match"):
        _w().read_glwe_ciphertext(FP, _glwe_bytes(glwes[0], 2 * P.N))
    with pytest.raises(E, match="does not match"):
        _w().read_glwe_ciphertext(FP, _glwe_bytes(glwes[0].reshape(-1)[:-P.N], P.N))     # GLWE size 2 under a k = 2 set
    with pytest.raises(E, match="longer than the destination"):
        _w().read_glwe_ciphertext(FP, _glwe_bytes(np.zeros((P.k + 2) * P.N, dtype=np.uint64), P.N))
    with pytest.raises(E):
        _w().write_glwe_ciphertext(FP, glwes[0].reshape(-1)[:-1])


def test_packed_results_travel():
    """What a server sends back: pack on the host, serialize, read, decrypt."""
    p = O.TOY_K1
    FP = to_fhestr_params(p)
    ck = _f().ClientKey(FP, 0x5EED0400)
    pp, key = ck.gen_packing_key(seed=3)
    pp2, key2 = _w().read_packing_key(FP, _w().write_packing_key(FP, pp, key))
    msgs = np.arange(300) % (p.msg_mod * p.carry_mod)
    glwes = _f().packing_keyswitch_host(FP, pp2, key2, ck.encrypt(msgs))
    back = _w().read_glwe_list(FP, _w().write_glwe_list(FP, glwes))
    assert np.array_equal(ck.decrypt_packed(back, 300), msgs)
    ck.close()
