"""The reference's compact-public-key parameter sets (tests/golden/reference_parameter_sets_compact_pk.json: the 56
constants of shortint/parameters/parameters_compact_pk.rs) on the GPU with their real dimensions.  tests/test_parameter_tables.py
checks, without a device, which of them fhe_params_supported accepts; here every accepted one gets keys and runs.

They bring shapes the classic table (tests/test_gpu_parameter_sets.py) lacks: n = 1024 (1025 keyswitch columns) in
PBS -> KS order; keyswitch decompositions of 11 x base 2 and 22 x base 1 levels at N = 32768 / 16384, whose key has
k N ks_level / 4 = 90112 row quads -- more than one launch of ksk_pack_kernel may cover (Engine::install_keys loops over
the spans of csrc/grid_spans.h); three PBS levels at N = 16384 / 32768 with real n; msg * carry = 256.

  test_compact_pk_set_decrypts      one case per accepted set: device keygen, a random table, every message (64 random
                                    ones where msg * carry > 64), decrypt; the _PBS_KS sets in small-key order
  test_keyswitch_on_exported_keys   the keyswitch decompositions no classic set has, and the two 90112-quad sets: the device's
                                    keyswitch of 4 encryptions and the 14 edge rows under the EXPORTED device key, bit for
                                    bit against ExactKeyswitch
  test_compact_lists_on_their_sets  N = 2048, 8192, 32768: expand_compact_list word for word against fhe_compact_expand_host
                                    for 1, k N and k N + 1 ciphertexts of a list encrypted with the public key; expanded rows
                                    (the first, the last of the first bin, the one alone in the second) through a table, decrypted"""
import dataclasses
import json
import os

import numpy as np
import pytest

from exact_keyswitch import N_EDGE_ROWS, ExactKeyswitch, edge_big_cts

pytestmark = pytest.mark.gpu

TABLE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_parameter_sets_compact_pk.json")))


def _params(name):
    import fhestr
    r = TABLE[name]
    return fhestr.Params(r["lwe_dimension"], r["glwe_dimension"], r["polynomial_size"], r["pbs_base_log"], r["pbs_level"],
                         r["ks_base_log"], r["ks_level"], r["message_modulus"], r["carry_modulus"],
                         r["lwe_modular_std_dev"], r["glwe_modular_std_dev"], name, r.get("grouping_factor", 0))


def _accepted():
    import fhestr
    return sorted(name for name in TABLE if fhestr.params_supported(_params(name))[0])


ACCEPTED = _accepted()


def _small_key_order(name):
    return TABLE[name]["encryption_key_choice"] == "Small"


def test_accepted_sets_are_the_ones_the_table_test_counts():
    assert len(TABLE) == 56 and len(ACCEPTED) == 39
    assert sum(_small_key_order(n) for n in ACCEPTED) == 12 and all(n.endswith("_PBS_KS") == _small_key_order(n) for n in ACCEPTED)
    quads = {n: TABLE[n]["glwe_dimension"] * TABLE[n]["polynomial_size"] * TABLE[n]["ks_level"] // 4 for n in ACCEPTED}
    assert sorted(n for n, q in quads.items() if q > 65535) == QUADS_90112 and all(quads[n] == 90112 for n in QUADS_90112)


def _lookup(eng, name, cts, idx):
    """One table over big-key ciphertexts in the set's own order.  PBS -> KS order (shortint/server_key/mod.rs:859-932) works on
    small-key ciphertexts and the client encrypts under the big key, so: keyswitch in, PBS + KS with the table, identity
    PBS out to a big-key ciphertext."""
    if not _small_key_order(name):
        return eng.apply_lookup_table(cts, idx)
    ident, _ = eng.generate_lookup_table(lambda x: x)
    small = eng.apply_lookup_table_small_key(eng.keyswitch(cts), idx)
    return eng.pbs(small, np.full(len(cts), ident, dtype=np.uint32))


@pytest.mark.parametrize("name", ACCEPTED)
def test_compact_pk_set_decrypts(name):
    import fhestr
    P = _params(name)
    M = P.msg_mod * P.carry_mod
    ck = fhestr.ClientKey(P, 0xC5E7)
    g, s = ck.secret_keys()
    eng = fhestr.Engine(P, 0)
    try:
        eng.generate_keys(g, s, 0xC5E7)
        rng = np.random.default_rng(13)
        table = rng.integers(0, M, size=M)
        lut, _ = eng.generate_lookup_table(lambda x: int(table[x]))
        msgs = np.arange(max(M, 8)) % M if M <= 64 else rng.integers(0, M, size=64)
        out = _lookup(eng, name, ck.encrypt(msgs), np.full(len(msgs), lut, dtype=np.uint32))
        assert np.array_equal(ck.decrypt(out), table[msgs])
    finally:
        eng.close()


# ---- the keyswitch on exported device keys ------------------------------------------------------------------------------------

QUADS_90112 = ["PARAM_MESSAGE_1_CARRY_7_COMPACT_PK_PBS_KS", "PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_PBS_KS"]
# (levels, base_log) -> a set that has it; none of these pairs is in tests/golden/reference_parameter_sets.json at n = 1024
NEW_DECOMPOSITIONS = {(11, 2): "PARAM_MESSAGE_4_CARRY_1_COMPACT_PK_PBS_KS", (22, 1): "PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_PBS_KS",
                      (7, 3): "PARAM_MESSAGE_3_CARRY_3_COMPACT_PK_PBS_KS", (5, 4): "PARAM_MESSAGE_1_CARRY_6_COMPACT_PK_PBS_KS",
                      (4, 5): "PARAM_MESSAGE_3_CARRY_2_COMPACT_PK_PBS_KS"}
KS_SETS = sorted(set(NEW_DECOMPOSITIONS.values()) | set(QUADS_90112))


def test_keyswitch_sets_have_the_decompositions_they_stand_for():
    for (level, base_log), name in NEW_DECOMPOSITIONS.items():
        r = TABLE[name]
        assert (r["ks_level"], r["ks_base_log"], r["lwe_dimension"]) == (level, base_log, 1024) and name in ACCEPTED
    assert set(QUADS_90112) <= set(ACCEPTED) and len(KS_SETS) == 6


def _exact_keyswitch(p, ksk, cts, block=128):
    """ExactKeyswitch over blocks of key columns (a 2.75 GB key as four float64 limb matrices would be 11 GB at once): the sum
    of a column reads that column of the key alone; the body lands in the last column, so only the last block sees it."""
    in_dim, out = p.k * p.N, p.n + 1
    ksk = ksk.reshape(in_dim * p.ks_level, out)
    no_body = cts.copy()
    no_body[:, in_dim] = 0
    parts = []
    for c0 in range(0, out, block):
        c1 = min(out, c0 + block)
        sub = dataclasses.replace(p, n=c1 - c0 - 1)
        parts.append(ExactKeyswitch(sub, np.ascontiguousarray(ksk[:, c0:c1]))(cts if c1 == out else no_body))
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("name", KS_SETS)
def test_keyswitch_on_exported_keys(name):
    import fhestr
    import oracle as O
    P = _params(name)
    p = O.Params(P.n, P.k, P.N, P.pbs_base_log, P.pbs_level, P.ks_base_log, P.ks_level, P.msg_mod, P.carry_mod, P.lwe_std, P.glwe_std, name)
    M = P.msg_mod * P.carry_mod
    ck = fhestr.ClientKey(P, 0xC5E8)
    g, s = ck.secret_keys()
    eng = fhestr.Engine(P, 0)
    try:
        _, ksk = eng.generate_keys(g, s, 0xC5E8, export=True)
        cts = np.concatenate([ck.encrypt(np.array([0, M - 1, M // 2, 1])), edge_big_cts(p, np.random.default_rng([P.N, P.ks_level]), N_EDGE_ROWS)])
        got = eng.keyswitch(cts)
        info = eng.keyswitch_info()
        print(f"{name}: {P.ks_level} levels of base 2^{P.ks_base_log}, {P.k * P.N * P.ks_level // 4} row quads, {info}")
        assert info["kernel"] == ("mfma" if P.ks_level <= 16 else "dot4")
        want = _exact_keyswitch(p, np.asarray(ksk, dtype=np.uint64), cts)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{len(bad)} of {want.size} words differ from exact; first (row, column) {bad[:12].tolist()}"
    finally:
        eng.close()


# ---- compact public keys on sets made for them ---------------------------------------------------------------------------------

PK_SETS = ["PARAM_MESSAGE_2_CARRY_2_COMPACT_PK_KS_PBS", "PARAM_MESSAGE_1_CARRY_5_COMPACT_PK_PBS_KS", "PARAM_MESSAGE_1_CARRY_7_COMPACT_PK_PBS_KS"]


def test_public_key_sets_cover_the_three_sizes():
    assert [TABLE[n]["polynomial_size"] for n in PK_SETS] == [2048, 8192, 32768] and set(PK_SETS) <= set(ACCEPTED)


@pytest.mark.parametrize("name", PK_SETS)
def test_compact_lists_on_their_sets(name):
    import fhestr
    P = _params(name)
    M, dim = P.msg_mod * P.carry_mod, P.k * P.N
    ck = fhestr.ClientKey(P, 0xC5E9)
    pk = ck.compact_public_key(0x9B11D)
    g, s = ck.secret_keys()
    eng = fhestr.Engine(P, 0)
    try:
        rng = np.random.default_rng([P.N, 14])
        for count in (1, dim, dim + 1):
            msgs = rng.integers(0, P.msg_mod, size=count, dtype=np.uint64)
            clist = pk.encrypt(msgs, count)
            assert clist.size == fhestr.compact_list_len(P, count) == -(-count // dim) * dim + count
            got = eng.expand_compact_list(clist, count)
            assert got.shape == (count, dim + 1)
            assert np.array_equal(got, fhestr.expand_compact_host(P, clist, count)), f"{count} ciphertexts"
            if count <= dim:
                del got                                          # 8.6 GB at N = 32768: gone before the next call's
        pick = np.array([0, 1, dim // 2, dim - 1, dim])          # the last call: first bin's ends, and the one row of the second bin
        assert np.array_equal(ck.decrypt(got[pick]), msgs[pick].astype(np.int64))
        cts = got[pick].copy()
        del got
        eng.generate_keys(g, s, 0xC5E9)
        table = rng.integers(0, M, size=M)
        lut, _ = eng.generate_lookup_table(lambda x: int(table[x]))
        out = _lookup(eng, name, cts, np.full(len(pick), lut, dtype=np.uint32))
        assert np.array_equal(ck.decrypt(out), table[msgs[pick].astype(np.int64)])
    finally:
        eng.close()
