"""Trivium and Kreyvium in the clear (csrc/stream_cipher.cpp behind fhe_stream_cipher_keystream): a model written here from
the ciphers' equations reproduces the key / IV / keystream vectors of the reference's apps/trivium tests
(tests/golden/stream_cipher_vectors.json), and the library equals the model on the vectors, on random keys and from a nonzero
first byte.  No device needed."""
import json
import os

import numpy as np
import pytest

import fhestr

VECTORS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_cipher_vectors.json")))
CIPHERS = ("trivium", "kreyvium")


def model_keystream(cipher, key: bytes, iv: bytes, n_bytes: int, first_byte: int = 0) -> bytes:
    """The history form: a[t], b[t], c[t] is the bit shifted into A, B, C at step t; a[-i] = s_i, b[-i] = s_{93+i},
    c[-i] = s_{177+i}.  Lists indexed at t + 128."""
    L = 80 if cipher == "trivium" else 128
    bits = lambda by: [(by[i >> 3] >> (i & 7)) & 1 for i in range(L)]
    x_key, x_iv = bits(key), bits(iv)
    K = lambda j: x_key[L - j]                  # spec bit K_j, 1 .. L
    IV = lambda j: x_iv[L - j]
    s = [0] * 289                               # s[1 .. 288]
    if cipher == "trivium":
        for j in range(1, 81):
            s[j], s[93 + j] = K(j), IV(j)
        s[286] = s[287] = s[288] = 1
    else:
        for j in range(1, 94):
            s[j] = K(j)
        for j in range(1, 85):
            s[93 + j] = IV(j)
        for j in range(85, 129):
            s[177 + j - 84] = IV(j)
        for j in range(222, 288):
            s[j] = 1
    O = 128
    steps = 1152 + 8 * (first_byte + n_bytes)
    a, b, c = ([0] * (O + steps) for _ in range(3))
    for i in range(1, 94):
        a[O - i] = s[i]
    for i in range(1, 85):
        b[O - i] = s[93 + i]
    for i in range(1, 112):
        c[O - i] = s[177 + i]
    z = [0] * steps
    for t in range(steps):
        u = O + t
        kt, ivt = (K(t % 128 + 1), IV(t % 128 + 1)) if cipher == "kreyvium" else (0, 0)
        z[t] = a[u - 66] ^ a[u - 93] ^ b[u - 69] ^ b[u - 84] ^ c[u - 66] ^ c[u - 111] ^ kt
        a[u] = c[u - 66] ^ c[u - 111] ^ (c[u - 109] & c[u - 110]) ^ a[u - 69] ^ kt
        b[u] = a[u - 66] ^ a[u - 93] ^ (a[u - 91] & a[u - 92]) ^ b[u - 78] ^ ivt
        c[u] = b[u - 69] ^ b[u - 84] ^ (b[u - 82] & b[u - 83]) ^ c[u - 87]
    ks = z[1152 + 8 * first_byte:]
    return bytes(sum(ks[8 * j + l] << l for l in range(8)) for j in range(n_bytes))


def _cases():
    return [(c, v["name"], bytes.fromhex(v["key"]), bytes.fromhex(v["iv"]), v["windows"]) for c in CIPHERS for v in VECTORS[c]]


def test_the_fixture_holds_what_the_reference_tests_hold():
    assert [len(VECTORS[c]) for c in CIPHERS] == [4, 4]
    assert sorted(w["first_byte"] for w in VECTORS["trivium"][0]["windows"]) == [0, 192, 256, 448]
    assert all(w["first_byte"] + len(w["keystream"]) // 2 <= 512 for c in CIPHERS for v in VECTORS[c] for w in v["windows"])


@pytest.mark.parametrize("cipher,name,key,iv,windows", _cases(), ids=[c[1] for c in _cases()])
def test_model_and_library_reproduce_the_vectors(cipher, name, key, iv, windows):
    for w in windows:
        want = bytes.fromhex(w["keystream"])
        assert model_keystream(cipher, key, iv, len(want), w["first_byte"]) == want
        assert fhestr.stream_keystream(cipher, key, iv, len(want), w["first_byte"]) == want


@pytest.mark.parametrize("cipher", CIPHERS)
def test_library_equals_model_on_random_keys(cipher):
    rng = np.random.default_rng(0x5C1F + len(cipher))
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    for _ in range(20):
        key, iv = rng.bytes(n), rng.bytes(n)
        assert fhestr.stream_keystream(cipher, key, iv, 200) == model_keystream(cipher, key, iv, 200)


@pytest.mark.parametrize("cipher", CIPHERS)
def test_a_nonzero_first_byte_continues_the_stream(cipher):
    rng = np.random.default_rng(7)
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    key, iv = rng.bytes(n), rng.bytes(n)
    whole = fhestr.stream_keystream(cipher, key, iv, 100)
    for first in (1, 8, 37, 99):
        assert fhestr.stream_keystream(cipher, key, iv, 100 - first, first) == whole[first:]
    assert fhestr.stream_keystream(cipher, key, iv, 13, 37) == model_keystream(cipher, key, iv, 13, 37)
    assert fhestr.stream_keystream(cipher, key, iv, 0, 5) == b""


@pytest.mark.parametrize("cipher", CIPHERS)
def test_stream_encrypt_is_an_involution(cipher):
    rng = np.random.default_rng(11)
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    key, iv, data = rng.bytes(n), rng.bytes(n), rng.bytes(77)
    for offset in (0, 8, 24):
        ct = fhestr.stream_encrypt(cipher, key, iv, data, offset)
        assert ct != data and len(ct) == len(data)
        assert fhestr.stream_encrypt(cipher, key, iv, ct, offset) == data
        ks = fhestr.stream_keystream(cipher, key, iv, len(data), offset)
        assert ct == bytes(x ^ y for x, y in zip(data, ks))


def test_info_and_refusals():
    assert fhestr.stream_cipher_info("trivium") == {"key_bits": 80, "iv_bits": 80, "warmup_steps": 1152}
    assert fhestr.stream_cipher_info("kreyvium") == {"key_bits": 128, "iv_bits": 128, "warmup_steps": 1152}
    with pytest.raises(fhestr.FheError, match="unknown stream cipher"):
        fhestr.stream_cipher_info("rc4")
    with pytest.raises(fhestr.FheError, match="10 bytes"):
        fhestr.stream_keystream("trivium", bytes(16), bytes(10), 8)
    with pytest.raises(fhestr.FheError, match="16 bytes"):
        fhestr.stream_keystream("kreyvium", bytes(16), bytes(10), 8)
