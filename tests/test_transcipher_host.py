"""The homomorphic Trivium / Kreyvium round without any crypto (csrc/transcipher.cpp, csrc/transcipher.h): the host
restatement of init, gather and apply runs on trivial ciphertexts with every lookup read from the tables the ABI exports,
and must give exactly data xor keystream in block form -- which pins taps, multipliers, complemented tables, ring indexing
across the wrap and the block layout.  Plus: which parameter sets are accepted, the wide-open-value bound of every table,
and the same units stand-alone under AddressSanitizer + UBSan (tests/transcipher_main.cpp; nothing loaded into Python).
No device needed."""
import os
import subprocess

import numpy as np
import pytest

import fhestr
import oracle as O
from conftest import to_fhestr_params
from transcipher_ref import WIDTHS, ClearLookupRun, HostSteps, plain_blocks, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fhe-string-bounty_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "transcipher_main.cpp"), os.path.join(CSRC, "stream_cipher.cpp"), os.path.join(CSRC, "transcipher.cpp")]
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")
CIPHERS = ("trivium", "kreyvium")
ACCEPTED = (to_fhestr_params(O.TOY_K1), fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS, fhestr.PARAM_MESSAGE_4_CARRY_4_KS_PBS)
FOUR_VALUES = (to_fhestr_params(O.TOY_K2), fhestr.PARAM_MESSAGE_1_CARRY_1_KS_PBS, fhestr.PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS,
               fhestr.PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS)


@pytest.mark.parametrize("streams", (1, 3))
@pytest.mark.parametrize("cipher", CIPHERS)
def test_round_restatement_on_trivial_ciphertexts(cipher, streams):
    """Full warm-up and 4 data rounds in two calls (11 bytes at keystream byte 0, 16 at byte 16)."""
    P = to_fhestr_params(O.TOY_K1)
    rng = np.random.default_rng(0x7C + 10 * streams + len(cipher))
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    key, ivs = rng.bytes(n), [rng.bytes(n) for _ in range(streams)]
    run = ClearLookupRun(P, cipher, fhestr.stream_key_bits(cipher, key), HostSteps(P)).begin(ivs)
    assert run.round == 18
    offset = 0
    for n_bytes in (11, 16):
        plain = [rng.bytes(n_bytes) for _ in range(streams)]
        got = run.next([fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plain)])
        want = np.stack([fhestr.string_to_blocks(P, s, n_bytes) for s in plain])
        assert np.array_equal(got, want.astype(np.int64))
        offset += 8 * -(-n_bytes // 8)
    assert run.round == 22
    assert run.max_input == (14 if cipher == "kreyvium" else 11)


@pytest.mark.parametrize("streams", (1, 3))
@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("shape_name", WIDTHS)
def test_round_restatement_at_every_block_width(shape_name, cipher, streams):
    """The same run at 1, 2, 4 and 8 bits per block, calls of 13 and then 40 bytes: m reaches 4 and the data rounds lap the
    ring (rounds 18 .. 24).  The expected blocks are shifts and masks of the plaintext bytes, not the library's."""
    P = shape(shape_name)
    assert fhestr.transcipher_supported(P, cipher) == (True, "")
    rng = np.random.default_rng(0x81D + 10 * streams + len(cipher) + P.msg_mod)
    n = fhestr.stream_cipher_info(cipher)["key_bits"] // 8
    key, ivs = rng.bytes(n), [rng.bytes(n) for _ in range(streams)]
    run = ClearLookupRun(P, cipher, fhestr.stream_key_bits(cipher, key), HostSteps(P)).begin(ivs)
    assert run.round == 18
    offset = 0
    for n_bytes in (13, 40):
        plain = [rng.bytes(n_bytes) for _ in range(streams)]
        got = run.next([fhestr.stream_encrypt(cipher, key, iv, s, offset) for iv, s in zip(ivs, plain)])
        assert got.shape == (streams, n_bytes * 8 // (P.msg_mod.bit_length() - 1))
        assert np.array_equal(got, np.stack([plain_blocks(P, s) for s in plain]))
        assert np.array_equal(got, np.stack([fhestr.string_to_blocks(P, s, n_bytes) for s in plain]).astype(np.int64))
        offset += 8 * -(-n_bytes // 8)
    assert run.round == 18 + 2 + 5
    assert run.max_input == (14 if cipher == "kreyvium" else 11)


def test_a_wrong_iv_or_offset_gives_another_string():
    """The check above can tell: the same loop under another IV, or data encrypted at another offset, does not decrypt."""
    P = to_fhestr_params(O.TOY_K1)
    key, iv, plain = bytes(range(16)), bytes(range(16, 32)), b"eight ch"
    want = fhestr.string_to_blocks(P, plain, 8).astype(np.int64)
    run = lambda iv2, off: ClearLookupRun(P, "kreyvium", fhestr.stream_key_bits("kreyvium", key), HostSteps(P)).begin([iv2]).next(
        [fhestr.stream_encrypt("kreyvium", key, iv, plain, off)])[0]
    assert np.array_equal(run(iv, 0), want)
    assert not np.array_equal(run(bytes(16), 0), want)
    assert not np.array_equal(run(iv, 8), want)


@pytest.mark.parametrize("cipher", CIPHERS)
def test_supported_and_refused_parameter_sets(cipher):
    for P in ACCEPTED:
        assert fhestr.transcipher_supported(P, cipher) == (True, ""), P.name
    for P in FOUR_VALUES:
        ok, why = fhestr.transcipher_supported(P, cipher)
        assert not ok and "msg_mod * carry_mod = 4" in why and "16 needed" in why, (P.name, why)
    ok, why = fhestr.transcipher_supported(fhestr.PARAM_MESSAGE_2_CARRY_1_KS_PBS, cipher)      # 8 values
    assert not ok and "msg_mod * carry_mod = 8" in why
    ok, why = fhestr.transcipher_supported(fhestr.PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS, cipher)   # 3-bit blocks
    assert not ok and "divide" in why
    with pytest.raises(fhestr.FheError, match="unknown stream cipher"):
        fhestr.transcipher_supported(ACCEPTED[0], 3)
    with pytest.raises(fhestr.FheError, match="16 needed"):
        fhestr.transcipher_tables(FOUR_VALUES[0])


# What the gate answers over the reference's parameter table (tests/golden/reference_parameter_sets.json), by name without
# the PARAM_ prefix; a name without _KS_PBS / _PBS_KS stands for every set that starts with it.
GATE_BOTH = ("MESSAGE_1_CARRY_3", "MESSAGE_1_CARRY_4", "MESSAGE_1_CARRY_5", "MESSAGE_1_CARRY_6", "MESSAGE_1_CARRY_7", "MESSAGE_2_CARRY_2_KS_PBS",
             "MESSAGE_2_CARRY_3", "MESSAGE_2_CARRY_4", "MESSAGE_2_CARRY_5", "MESSAGE_2_CARRY_6", "MESSAGE_4_CARRY_0", "MESSAGE_4_CARRY_2",
             "MESSAGE_4_CARRY_3", "MESSAGE_4_CARRY_4_KS_PBS", "MESSAGE_4_CARRY_4_PBS_KS", "MESSAGE_8_CARRY_0")
GATE_TRIVIUM_ONLY = ("MESSAGE_2_CARRY_2_PBS_KS",)
GATE_TOO_NOISY = ("MESSAGE_4_CARRY_1", "MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2", "MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3")
GATE_WIDTH = ("MESSAGE_3_CARRY_1", "MESSAGE_3_CARRY_2", "MESSAGE_3_CARRY_3_KS_PBS", "MESSAGE_3_CARRY_3_PBS_KS", "MESSAGE_3_CARRY_4", "MESSAGE_3_CARRY_5",
              "MESSAGE_5_CARRY_0", "MESSAGE_5_CARRY_1", "MESSAGE_5_CARRY_2", "MESSAGE_5_CARRY_3", "MESSAGE_6_CARRY_0", "MESSAGE_6_CARRY_1",
              "MESSAGE_6_CARRY_2", "MESSAGE_7_CARRY_0", "MESSAGE_7_CARRY_1", "MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2", "MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3")
GATE_FEW_VALUES = ("MESSAGE_1_CARRY_0", "MESSAGE_1_CARRY_1_KS_PBS", "MESSAGE_1_CARRY_1_PBS_KS", "MESSAGE_1_CARRY_2", "MESSAGE_2_CARRY_0", "MESSAGE_2_CARRY_1",
                   "MESSAGE_3_CARRY_0", "MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2", "MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3")
# nominal variances of the lookup inputs of registers a, b, c and of a keystream row (csrc/transcipher.h): 2 (T + 1)^2 + T, 6 or 7
GATE_NOISE = {"trivium": (35, 35, 35, 6), "kreyvium": (54, 35, 35, 7)}


def _gate_rule(P, cipher) -> bool:
    """The noise part of the gate restated from the model's variances: every row kind's noise is at most max(max_level^2,
    budget), budget = the nu the model gives log2 p_fail(max_level^2) + slack, V_pbs times 4 on shapes nobody measured,
    slack half a bit and none for grouping factor 2 (csrc/noise_model.h, default_noise_budget)."""
    import math
    m = fhestr.noise_model(P)
    v_pbs = m["v_pbs"] * (1.0 if fhestr.noise_model_is_calibrated(P) else 4.0)

    def log2_pfail(nu):
        z = m["half_box"] / math.sqrt(nu * v_pbs + m["v_ks"] + m["v_ms"])
        p = math.erfc(z / math.sqrt(2.0))
        return math.log2(p) if p > 1e-300 else (-(z * z) / 2 - math.log(z * math.sqrt(math.pi / 2))) / math.log(2.0)

    ref_nu = ((P.msg_mod * P.carry_mod - 1) / (P.msg_mod - 1)) ** 2
    target = log2_pfail(ref_nu) + (0.0 if P.grouping == 2 else 0.5)
    return all(nu <= ref_nu or log2_pfail(nu) <= target for nu in GATE_NOISE[cipher])     # log2 p_fail rises with nu


def test_the_gate_over_the_reference_parameter_table():
    """Every entry of the reference's table, both ciphers, against the lists above; and the accepted ones among the sets with
    16 values and a legal width are exactly those the rule restated in _gate_rule lets through."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from noise_budget import reference_params
    names = sorted(json.load(open(os.path.join(ROOT, "tests", "golden", "reference_parameter_sets.json"))))
    assert len(names) == 46
    listed = {}
    for verdict, group in (("both", GATE_BOTH), ("trivium", GATE_TRIVIUM_ONLY), ("nominal variances", GATE_TOO_NOISY), ("divide", GATE_WIDTH),
                           ("16 needed", GATE_FEW_VALUES)):
        for prefix in group:
            hits = [n for n in names if n == "PARAM_" + prefix or n.startswith("PARAM_" + prefix + "_")]
            assert hits, prefix
            for n in hits:
                assert n not in listed, n
                listed[n] = verdict
    assert sorted(listed) == names
    assert sum(v == "both" for v in listed.values()) == 16
    for name in names:
        P, verdict = reference_params(name), listed[name]
        for cipher in CIPHERS:
            ok, why = fhestr.transcipher_supported(P, cipher)
            if verdict == "both" or (verdict == "trivium" and cipher == "trivium"):
                assert (ok, why) == (True, ""), (name, cipher, why)
            else:
                want = "nominal variances" if verdict == "trivium" else verdict
                assert not ok and want in why, (name, cipher, why)
            values, bits = P.msg_mod * P.carry_mod, P.msg_mod.bit_length() - 1
            if values >= 16 and bits in (1, 2, 4, 8):
                assert ok == _gate_rule(P, cipher), (name, cipher, why)
            else:
                assert verdict == ("16 needed" if values < 16 else "divide"), name


def test_refused_when_the_noise_budget_is_too_small():
    """A 16-value set whose noise the model does not accept is refused with the figures."""
    from dataclasses import replace
    noisy = replace(fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS, glwe_std=3e-14, name="noisy")
    budget = fhestr.noise_model(noisy)["budget"]
    assert budget < 35, budget
    for cipher, nu in (("trivium", 35), ("kreyvium", 54)):
        ok, why = fhestr.transcipher_supported(noisy, cipher)
        assert not ok and f"carries {nu} nominal variances" in why and "budget" in why, why


@pytest.mark.parametrize("P", ACCEPTED + tuple(shape(w) for w in WIDTHS if w != "W2"), ids=lambda P: P.name)      # W2 is TOY_K1
def test_wide_open_value_bound_and_table_semantics(P):
    """Every v = (T + 1) s + t over all s in 0..2 and t in 0..T stays below msg * carry, and the table at v is
    (x and y) xor parity(t) -- complemented for the complemented table; g_{i,c} is ((v & 1) xor c) << i for v <= 7."""
    M, bits = P.msg_mod * P.carry_mod, P.msg_mod.bit_length() - 1
    tables = fhestr.transcipher_tables(P)
    assert all(fhestr.transcipher_supported(P, c) == (True, "") for c in CIPHERS)
    assert tables.shape == (4 + 2 * bits, M)
    for T, base in ((3, 0), (4, 2)):
        seen = set()
        for s in range(3):
            for t in range(T + 1):
                v = (T + 1) * s + t
                assert v < M
                seen.add(v)
                want = int(s == 2) ^ (t & 1)
                assert tables[base, v] == want and tables[base + 1, v] == 1 - want
        assert max(seen) == (11 if T == 3 else 14) and len(seen) == 3 * (T + 1)
    for i in range(bits):
        for c in (0, 1):
            for v in range(8):
                assert v < M and tables[4 + 2 * i + c, v] == ((v & 1) ^ c) << i
    assert tables.max() < P.msg_mod


def test_encrypt_stream_key_gives_the_bits_in_spec_order():
    P = to_fhestr_params(O.TOY_K1)
    ck = fhestr.ClientKey(P, 5)
    for cipher, L in (("trivium", 80), ("kreyvium", 128)):
        key = bytes((37 * i + 11) % 256 for i in range(L // 8))
        cts = ck.encrypt_stream_key(cipher, key)
        assert cts.shape == (L, P.big_size)
        bits = ck.decrypt(cts)
        assert all(int(bits[j - 1]) == (key[(L - j) >> 3] >> ((L - j) & 7)) & 1 for j in range(1, L + 1))
    with pytest.raises(fhestr.FheError, match="16 bytes"):
        ck.encrypt_stream_key("kreyvium", bytes(10))


def test_stand_alone_program_under_host_sanitizers(tmp_path):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    assert cxx is not None, "no host C++ compiler found: " + ", ".join(COMPILERS)
    program = str(tmp_path / "transcipher_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-o", program, *SOURCES, "-lm"], check=True)
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert lines == [f"ok cipher {c} streams {s} rounds 22" for _ in range(4) for c in (1, 2) for s in (1, 3)]      # four shapes: 2, 4, 1 and 8 bits
