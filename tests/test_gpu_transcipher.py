"""Transciphering on the GPU (csrc/transcipher_kernels.hip.h, csrc/transcipher_dev.hip): the three kernels against the host
restatement word for word on random rows, then Trivium- and Kreyvium-encrypted strings turned into encrypted strings end to
end on TOY_K1, one Kreyvium string on PARAM_MESSAGE_2_CARRY_2 fed to string operations, and the refusals."""
import numpy as np
import pytest

import fhestr
from conftest import gpu_engine

pytestmark = pytest.mark.gpu

CIPHERS = ("trivium", "kreyvium")


def _dec(ks, cts):
    return ks.ck.decrypt_many(np.asarray(cts).reshape(-1, ks.params.big_size))


def _key_cts(ks, cipher, key):
    return ks.ck.encrypt_many(fhestr.stream_key_bits(cipher, key))


def _material(cipher, streams, seed):
    rng = np.random.default_rng(seed)
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    return rng, rng.bytes(n), [rng.bytes(n) for _ in range(streams)]


@pytest.mark.parametrize("streams", (1, 3))
@pytest.mark.parametrize("cipher", CIPHERS)
def test_kernels_equal_the_host_restatement(toy_k1, cipher, streams):
    """Random u64 rows of TOY_K1 size in the ring and the key; warm-up rounds 0, 1, 3, 4, 5 (192 rows) and data rounds 18 .. 21
    and 23 (256 rows): every ring slot as a source and a wrap in both; table indices included."""
    eng = gpu_engine(toy_k1)
    P = eng.params
    rng, _, ivs = _material(cipher, streams, 0xA11CE + streams)
    L = fhestr.stream_cipher_info(cipher)["key_bits"]
    key = rng.integers(0, 2**64, size=(L, P.big_size), dtype=np.uint64)
    ring = rng.integers(0, 2**64, size=fhestr.transcipher_ring_len(P, streams), dtype=np.uint64)
    want = fhestr.transcipher_init_host(P, cipher, streams, key, ivs, ring)
    assert not np.array_equal(want, ring)
    assert np.array_equal(eng.transcipher_init(cipher, streams, key, ivs, ring), want)
    data = rng.bytes(streams * 11)
    for rows, rounds in ((192, (0, 1, 3, 4, 5)), (256, (18, 19, 20, 21, 23))):
        for r in rounds:
            for m in ((0,) if rows == 192 else (0, 1)):
                args = (cipher, streams, r, rows, ring, key, ivs, data if rows == 256 else None, m)
                w_in, w_tab = fhestr.transcipher_gather_host(P, *args)
                g_in, g_tab = eng.transcipher_gather(*args)
                assert np.array_equal(g_tab, w_tab), (r, rows, m)
                assert np.array_equal(g_in, w_in), (r, rows, m)
    assert len(np.unique(w_tab)) > 4                                  # keystream tables g_{i,c} among them
    bpc = fhestr.blocks_per_char(P)
    for r, n_bytes, m in ((18, 5, 0), (21, 11, 1), (23, 16, 0), (20, 16, 1)):
        out = rng.integers(0, 2**64, size=(streams * n_bytes * bpc, P.big_size), dtype=np.uint64)
        want = fhestr.transcipher_apply_host(P, cipher, streams, r, ring, n_bytes, m, out.copy())
        assert not np.array_equal(want, out)
        assert np.array_equal(eng.transcipher_apply(cipher, streams, r, ring, n_bytes, m, out.copy()), want), (r, n_bytes, m)


@pytest.mark.parametrize("streams", (1, 3))
@pytest.mark.parametrize("cipher", CIPHERS)
def test_end_to_end_on_toy_k1(toy_k1, cipher, streams):
    """begin, next of 5 bytes (keystream byte 0), next of 11 bytes (byte 8): decrypts to the plaintext with and without the
    refresh; a device destination holds the host output word for word."""
    import torch
    eng = gpu_engine(toy_k1)
    P = eng.params
    rng, key, ivs = _material(cipher, streams, 0xE2E + streams)
    assert len(set(ivs)) == streams
    tc = eng.transcipher(cipher, _key_cts(toy_k1, cipher, key), max_streams=3)
    plains = [[rng.bytes(n) for _ in range(streams)] for n in (5, 11)]
    bpc = fhestr.blocks_per_char(P)
    host = {}
    for refresh in (True, False):
        tc.begin(ivs)
        assert tc.offset == 0
        for call, (n, offset) in enumerate(((5, 0), (11, 8))):
            assert tc.offset == offset
            enc = [fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plains[call])]
            out = tc.next(enc, refresh=refresh)
            assert out.shape == (streams, n * bpc, P.big_size)
            for s in range(streams):
                assert fhestr.blocks_to_string(P, _dec(toy_k1, out[s])).ljust(n, b"\0") == plains[call][s]
                assert np.array_equal(_dec(toy_k1, out[s]), fhestr.string_to_blocks(P, plains[call][s], n))
            host[refresh, call] = out
        info = tc.info()
        assert (info["streams"], info["warmup_rounds"], info["data_rounds"], info["offset"]) == (streams, 18, 3, 24)
        assert info["pbs"] == streams * (18 * 192 + 3 * 256 + (16 * bpc if refresh else 0))
    assert not np.array_equal(host[True, 1], host[False, 1])
    tc.begin(ivs)
    for call, (n, offset) in enumerate(((5, 0), (11, 8))):
        enc = [fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plains[call])]
        d = torch.zeros((streams, n * bpc, P.big_size), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert tc.next(enc, d_out=d.data_ptr()) is None
        eng.synchronize()
        assert np.array_equal(d.cpu().numpy().view(np.uint64), host[True, call])
    tc.close()


def test_kreyvium_string_feeds_string_operations_on_p22(p22):
    """PARAM_MESSAGE_2_CARRY_2, one Kreyvium stream, a 16-character capacity: the result goes unchanged into contains and
    to_upper."""
    eng = gpu_engine(p22)
    P = eng.params
    ops = fhestr.FheStringOps(eng)
    _, key, (iv,) = _material("kreyvium", 1, 0x22)
    s = b"the quick fox"
    tc = eng.transcipher("kreyvium", _key_cts(p22, "kreyvium", key)).begin([iv])
    es = tc.next(fhestr.stream_encrypt("kreyvium", key, iv, s.ljust(16, b"\0")))
    assert es.shape == (16 * 4, P.big_size)
    assert fhestr.blocks_to_string(P, _dec(p22, es)) == s
    assert _dec(p22, ops.contains(es, b"quick"))[0] == 1
    assert _dec(p22, ops.contains(es, b"quack"))[0] == 0
    assert fhestr.blocks_to_string(P, _dec(p22, ops.to_upper(es))) == s.upper()
    info = tc.info()
    assert (info["warmup_rounds"], info["data_rounds"]) == (18, 2)
    assert info["pbs"] == 18 * 192 + 2 * 256 + 64
    tc.close()


def test_refusals_leave_the_object_usable(toy_k1):
    eng = gpu_engine(toy_k1)
    P = eng.params
    _, key, ivs = _material("trivium", 3, 0x4EF)
    cts = _key_cts(toy_k1, "trivium", key)
    with pytest.raises(fhestr.FheError, match="80 key-bit ciphertexts"):
        eng.transcipher("trivium", cts[:79])
    with pytest.raises(fhestr.FheError, match="128 key-bit ciphertexts"):
        eng.transcipher("kreyvium", cts)
    tc = eng.transcipher("trivium", cts, max_streams=2)
    with pytest.raises(fhestr.FheError, match="next before begin"):
        tc.next(b"abc")
    with pytest.raises(fhestr.FheError, match="3 streams.*1 .. 2"):
        tc.begin(ivs)
    with pytest.raises(fhestr.FheError, match="next before begin"):
        tc.next(b"abc")
    tc.begin(ivs[:1])
    with pytest.raises(fhestr.FheError, match="1 equally long"):
        tc.next([b"abc", b"abc"])
    plain = b"usable"
    out = tc.next(fhestr.stream_encrypt("trivium", key, ivs[0], plain))
    assert fhestr.blocks_to_string(P, _dec(toy_k1, out)) == plain
    with pytest.raises(fhestr.FheError, match="3 streams"):
        tc.begin(ivs)
    plain2 = b"still"
    out = tc.next(fhestr.stream_encrypt("trivium", key, ivs[0], plain2, tc.offset))
    assert fhestr.blocks_to_string(P, _dec(toy_k1, out)) == plain2
    tc.close()
