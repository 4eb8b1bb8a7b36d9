"""Transciphering on the GPU (csrc/transcipher_kernels.hip.h, csrc/transcipher_dev.hip): the three kernels against the host
restatement word for word on random rows, then Trivium- and Kreyvium-encrypted strings turned into encrypted strings end to
end on TOY_K1, one Kreyvium string on PARAM_MESSAGE_2_CARRY_2 fed to string operations, and the refusals.

Then every block width and real row lengths (the shapes of tests/transcipher_ref.py): the kernels against the host restatement
on rows of 1,537 and 2,049 words, the whole cipher through the kernels on trivial ciphertexts at 1, 2, 4 and 8 bits, end to end
with keys at 1 and 4 bits, and the noise of the real lookup inputs on PARAM_MESSAGE_2_CARRY_2 against the accounting of
csrc/transcipher.h.  Not pinned: 8 bits with keys, and rows of N >= 4096."""
import math
import os
import sys

import numpy as np
import pytest

import fhestr
import oracle as O
from conftest import ROOT, gpu_engine, keyset, to_fhestr_params
from transcipher_ref import (DATA_ROWS, KEYSTREAM, STATE_ROWS, WIDTHS, ClearLookupRun, EncryptedRun, GpuSteps, HostSteps, margin, oracle_shape, plain_blocks,
                             ring_row, shape, sources)

sys.path.insert(0, os.path.join(ROOT, "scripts"))

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


@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("shape_name", ("R2049", "R2049K2", "R1537", "W8"))
def test_kernels_equal_the_host_restatement_at_real_rows(shape_name, cipher):
    """Rows of 2,049 words (k = 1 and k = 2) and 1,537 words (k = 3): four and three trips of the 256 threads over a row's
    pairs, at 2, 4, 1 and 8 bits per block; one stream, no keys (the three entry points use none).  Warm-up rounds 0, 1, 3, 4, 5
    and data rounds 18 .. 21 and 23 with m in (0, 1, 4) over 37 bytes; every word and every table index; and the rows a kernel
    must leave alone come back as they were sent."""
    P = shape(shape_name)
    assert fhestr.transcipher_supported(P, cipher) == (True, "")
    eng = fhestr.Engine(P, 0)
    try:
        rng, _, ivs = _material(cipher, 1, 0xB16 + P.big_size + P.msg_mod)
        L = fhestr.stream_cipher_info(cipher)["key_bits"]
        key = rng.integers(0, 2**64, size=(L, P.big_size), dtype=np.uint64)
        sent = rng.integers(0, 2**64, size=fhestr.transcipher_ring_len(P, 1), dtype=np.uint64)
        ring = fhestr.transcipher_init_host(P, cipher, 1, key, ivs, sent)
        got = eng.transcipher_init(cipher, 1, key, ivs, sent)
        assert np.array_equal(got, ring)
        written = np.zeros(sent.size // P.big_size, dtype=bool)
        written[[ring_row(1, 0, reg, -i) for reg in range(3) for i in range(1, 129)]] = True
        assert written.sum() == 2 * STATE_ROWS
        rows_of = lambda a: a.reshape(-1, P.big_size)
        assert np.array_equal(rows_of(got)[~written], rows_of(sent)[~written])
        assert not (rows_of(got)[written] == rows_of(sent)[written]).all(axis=1).any()
        data = rng.bytes(37)
        seen = set()
        for rows, rounds in ((STATE_ROWS, (0, 1, 3, 4, 5)), (DATA_ROWS, (18, 19, 20, 21, 23))):
            for r in rounds:
                for m in ((0,) if rows == STATE_ROWS else (0, 1, 4)):
                    args = (cipher, 1, r, rows, ring, key, ivs, data if rows == DATA_ROWS else None, m)
                    w_in, w_tab = fhestr.transcipher_gather_host(P, *args)
                    g_in, g_tab = eng.transcipher_gather(*args)
                    assert np.array_equal(g_tab, w_tab), (r, rows, m)
                    assert np.array_equal(g_in, w_in), (r, rows, m)
                    seen.update(w_tab.reshape(-1).tolist())
        bits = P.msg_mod.bit_length() - 1
        assert {4 + 2 * i + c for i in range(bits) for c in (0, 1)} <= seen                # every keystream table g_{i,c} of the width
        bpc = fhestr.blocks_per_char(P)
        for r, n_bytes, m in ((18, 5, 0), (21, 11, 1), (23, 16, 0), (22, 37, 4)):
            out = rng.integers(0, 2**64, size=(n_bytes * bpc, P.big_size), dtype=np.uint64)
            want = fhestr.transcipher_apply_host(P, cipher, 1, r, ring, n_bytes, m, out.copy())
            got = eng.transcipher_apply(cipher, 1, r, ring, n_bytes, m, out.copy())
            assert np.array_equal(got, want), (r, n_bytes, m)
            mine = np.zeros(n_bytes * bpc, dtype=bool)
            mine[8 * m * bpc: min(8 * m + 8, n_bytes) * bpc] = True
            assert np.array_equal(got[~mine], out[~mine]) and not (got[mine] == out[mine]).all(axis=1).any(), (r, n_bytes, m)
    finally:
        eng.close()


@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("shape_name", WIDTHS)
def test_whole_cipher_through_the_kernels_on_trivial_ciphertexts(shape_name, cipher):
    """ClearLookupRun driven by the three kernels at 1, 2, 4 and 8 bits per block: 2 streams, calls of 13 and then 40 bytes
    (m up to 4, data rounds 18 .. 24 lap the ring).  The blocks are the plaintext's, and the final ring is the host run's word
    for word."""
    P = shape(shape_name)
    assert fhestr.transcipher_supported(P, cipher) == (True, "")
    eng = fhestr.Engine(P, 0)
    try:
        rng, key, ivs = _material(cipher, 2, 0xC1EA4 + P.msg_mod)
        bits = fhestr.stream_key_bits(cipher, key)
        gpu = ClearLookupRun(P, cipher, bits, GpuSteps(eng)).begin(ivs)
        host = ClearLookupRun(P, cipher, bits, HostSteps(P)).begin(ivs)
        offset = 0
        for n_bytes in (13, 40):
            plain = [rng.bytes(n_bytes) for _ in range(2)]
            enc = [fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plain)]
            want = np.stack([plain_blocks(P, s) for s in plain])
            assert np.array_equal(gpu.next(enc), want)
            assert np.array_equal(host.next(enc), want)
            offset += 8 * -(-n_bytes // 8)
        assert gpu.round == host.round == 25
        assert np.array_equal(gpu.ring, host.ring)
    finally:
        eng.close()


@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("shape_name", ("W1", "W4"))
def test_end_to_end_with_toy_keys_at_1_and_4_bits(shape_name, cipher):
    """begin, next of 13 bytes, next of 40 bytes on 2 streams, with and without the refresh: 8 blocks per character at 1 bit,
    2 at 4 bits.  8 bits gets no run with keys: the only accepted 8-bit shapes with a sound margin have N = 32768, where a
    warm-up alone is 3,456 bootstraps; the two tests above cover that width's kernels."""
    ks = keyset(oracle_shape(shape_name))
    P = to_fhestr_params(ks.params)
    assert fhestr.transcipher_supported(P, cipher) == (True, "")
    assert margin(P) >= 8                       # 8 sigma at 54 nominal variances: a lookup fails with probability 1e-15
    eng = fhestr.Engine(P, 0)
    try:
        eng.load_keys(ks.sk.bsk, ks.sk.ksk)
        rng, key, ivs = _material(cipher, 2, 0xE2E0 + P.msg_mod)
        tc = eng.transcipher(cipher, _key_cts(ks, cipher, key), max_streams=2)
        bpc = fhestr.blocks_per_char(P)
        assert bpc == {"W1": 8, "W4": 2}[shape_name]
        plains = [[rng.bytes(n) for _ in range(2)] for n in (13, 40)]
        for refresh in (True, False):
            tc.begin(ivs)
            for call, (n, offset) in enumerate(((13, 0), (40, 16))):
                assert tc.offset == offset
                enc = [fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plains[call])]
                out = tc.next(enc, refresh=refresh)
                assert out.shape == (2, n * bpc, P.big_size)
                for s in range(2):
                    assert np.array_equal(_dec(ks, out[s]), plain_blocks(P, plains[call][s]))
            info = tc.info()
            assert (info["streams"], info["warmup_rounds"], info["data_rounds"], info["offset"]) == (2, 18, 7, 56)
            assert info["pbs"] == 2 * (18 * 192 + 7 * 256 + (53 * bpc if refresh else 0))
        tc.close()
    finally:
        eng.close()


@pytest.mark.parametrize("name", ("PARAM_MESSAGE_1_CARRY_3_KS_PBS", "PARAM_MESSAGE_4_CARRY_0_KS_PBS"))
def test_kreyvium_string_on_real_rows_at_1_and_4_bits(name):
    """Two sets of the reference's table with N = 2048, k = 1, one level (PARAM_MESSAGE_2_CARRY_2's kernel family) at 1 and 4
    bits per block, keys generated on the device: one Kreyvium stream, 16 characters.  The sets are built for a failure
    probability of 2^-40 at their own worst case, about 7.3 sigma, so the 8 sigma of the toy shapes cannot be asked of them:
    7 sigma at 54 nominal variances is 2.6e-12 per lookup, 1e-8 over this test's 4,000 lookups."""
    from noise_budget import reference_params
    P = reference_params(name)
    assert (P.N, P.k, P.pbs_level) == (2048, 1, 1)
    assert fhestr.transcipher_supported(P, "kreyvium") == (True, "")
    assert margin(P) >= 7
    ck = fhestr.ClientKey(P, 0x5EED0C1F)
    eng = fhestr.Engine(P, 0)
    try:
        eng.generate_keys(*ck.secret_keys(), 0x5EED0C1F)
        _, key, (iv,) = _material("kreyvium", 1, 0x1604 + P.msg_mod)
        s = b"sixteen letters!"
        tc = eng.transcipher("kreyvium", ck.encrypt_stream_key("kreyvium", key)).begin([iv])
        es = tc.next(fhestr.stream_encrypt("kreyvium", key, iv, s))
        bpc = fhestr.blocks_per_char(P)
        assert es.shape == (16 * bpc, P.big_size)
        assert np.array_equal(ck.decrypt(es), plain_blocks(P, s))
        assert tc.info()["pbs"] == 18 * 192 + 2 * 256 + 16 * bpc
        tc.close()
    finally:
        eng.close()
        ck.close()


# nominal variances a lookup input gathers from PBS outputs, by row kind: 2 (T + 1)^2 + the XORed taps that are PBS outputs.
# Kreyvium's register a counts 53, not the 54 of csrc/transcipher.h: its fifth XORed term is the key row, a fresh encryption.
PBS_TAPS = {"trivium": (35, 35, 35, 6), "kreyvium": (53, 35, 35, 6)}
NOISE_STREAMS = 8


@pytest.mark.parametrize("cipher", CIPHERS)
def test_noise_at_the_lookup_inputs_on_p22(p22, cipher):
    """PARAM_MESSAGE_2_CARRY_2, 8 streams, rounds 0 .. 19 on real ciphertexts in lockstep with the clear run on the same key and
    IVs: every one of the 8 x (18 x 192 + 2 x 256) lookup outputs decrypts to the clear run's value.  At rounds 14 .. 17 (2,048
    inputs per register) and 18 .. 19 (1,024 keystream inputs), per row kind:
    (a) the second moment about zero of the input's big-key phase error over that of the ring rows it sums is 2 (T + 1)^2 + the
        PBS-output taps, within four standard errors of a ratio of two moment estimates, 4 sqrt(2 / n_in + 2 / n_src);
    (b) after the keyswitch and the modulus switch the spread is the model's within 8 %, the largest error stays below 0.8 of
        half a box, and the Gaussian log2 p_fail is at most -38: the bands of test_noise_model_against_measurement_per_kernel_family.
    The key bits are encrypted from a generator of their own, so the figures are the same in any test order.  Measured
    (profiles/transcipher_noise.txt): ratios within 10.3 % of the count -- the rows of a round share taps, so they scatter more
    than independent samples would -- and log2 p_fail -41.3 or lower."""
    from noise_budget import log2_pfail, small_key_errors
    eng = gpu_engine(p22)
    P, ck, S = eng.params, p22.ck, NOISE_STREAMS
    assert fhestr.transcipher_supported(P, cipher) == (True, "")
    assert margin(P) >= 7                       # a real set, 2^-40 at its own worst case: see the test above
    model = fhestr.noise_model(P)
    rng, key, ivs = _material(cipher, S, 0x9015E)
    tables = fhestr.transcipher_tables(P)
    luts = [eng.upload_lut(p22.sk.generate_lookup_table(lambda x, t=t: int(tables[t, x]))[0]) for t in range(len(tables))]
    clear = ClearLookupRun(P, cipher, fhestr.stream_key_bits(cipher, key), HostSteps(P)).start(ivs)
    key_cts = ck.encrypt_many(fhestr.stream_key_bits(cipher, key), O.Rng(0x9015E, 1))      # its own generator: the same figures in any test order
    enc = EncryptedRun(eng, cipher, key_cts, luts).begin(ivs)
    small_sel = np.flatnonzero(ck.small_sk.astype(np.uint64) == 1)
    delta = np.uint64(P.delta)

    def big_key_errors(rows, values):
        phase = np.array([ck.decrypt_plaintext(c) for c in rows], dtype=np.uint64)
        with np.errstate(over="ignore"):
            return (phase - np.asarray(values).astype(np.uint64) * delta).astype(np.int64).astype(np.float64) / 2.0**64

    e_in, e_ms, e_src = ({k: [] for k in range(4)} for _ in range(3))
    src_seen = {k: set() for k in range(4)}
    data = rng.bytes(S * 16)
    for r in range(20):
        rows = STATE_ROWS if r < 18 else DATA_ROWS
        pbs_in, tabs = enc.gather(rows, data if r >= 18 else None, r - 18 if r >= 18 else 0)
        clear._round(rows, np.frombuffer(data, dtype=np.uint8) if r >= 18 else None, r - 18 if r >= 18 else 0)
        assert np.array_equal(tabs, clear.last_tables), r
        kinds = (0, 1, 2) if 14 <= r < 18 else (KEYSTREAM,) if r >= 18 else ()
        if kinds:
            kind_of = np.arange(S * rows) % rows >> 6
            after_ms = small_key_errors(eng.keyswitch(pbs_in), clear.last_in.astype(np.uint64) * delta, small_sel, P.N)[1]
            clear_bits = clear.ring.reshape(-1, P.big_size)[:, -1] // delta
            for k in kinds:
                e_in[k].append(big_key_errors(pbs_in[kind_of == k], clear.last_in[kind_of == k]))
                e_ms[k].append(after_ms[kind_of == k])
                taps = {(s, reg, step) for s in range(S) for j in range(64) for reg, step, _ in sources(cipher, k, 64 * r + j)[0]} - src_seen[k]
                src_seen[k] |= taps
                at = [ring_row(S, *tap) for tap in sorted(taps)]
                e_src[k].append(big_key_errors(enc.rows(at), clear_bits[at]))
        out = enc.lookup(pbs_in, tabs)
        assert np.array_equal(ck.decrypt_many(out), clear.last_out), r
    half = model["half_box"]
    failures = []
    for k in range(4):
        a, b, src = (np.concatenate(x[k]) for x in (e_in, e_ms, e_src))
        assert a.size == b.size == (S * 64 * 4 if k < KEYSTREAM else S * 64 * 2)
        nu = PBS_TAPS[cipher][k]
        ratio, band = np.mean(a * a) / np.mean(src * src), 4 * math.sqrt(2 / a.size + 2 / src.size)
        model_std = math.sqrt(nu * model["v_pbs"] + model["v_ks"] + model["v_ms"])
        pfail = log2_pfail(float(b.std()), half)
        print(f"{cipher} kind {k}: n_in {a.size} n_src {src.size} ratio {ratio:.2f} (expected {nu}, band {100 * band:.1f} %) mean_in {a.mean():+.3e} "
              f"mean_src {src.mean():+.3e} std_src {src.std():.3e} | after KS+MS: std {b.std():.4e} (model {model_std:.4e}) mean {b.mean():+.3e} "
              f"max {np.abs(b).max():.3e} ({np.abs(b).max() / half:.2f} half box) log2 p_fail {pfail:.1f}")
        if abs(ratio / nu - 1) > band:
            failures.append((k, "ratio", ratio, nu, band))
        if abs(b.std() / model_std - 1) >= 0.08:
            failures.append((k, "std_after_ms", b.std(), model_std))
        if not np.abs(b).max() < 0.8 * half:
            failures.append((k, "max_abs_after_ms", np.abs(b).max(), half))
        if not pfail <= -38.0:
            failures.append((k, "log2_pfail", pfail))
    assert not failures, failures
