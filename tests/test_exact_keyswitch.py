"""tests/exact_keyswitch.py pinned on the CPU: the float64 limb form against the Python-integer loop and against the
oracle's keyswitch, on every keyswitch decomposition of the reference's parameter tables that the engine accepts and on
every edge input; and the edge inputs against what they claim to be."""
import json
import os

import numpy as np
import pytest

import oracle as O
from exact_keyswitch import (EDGE_KEY_WORDS, ExactKeyswitch, N_EDGE_ROWS, balanced_digits, closest_representable_int, decompose_int,
                             edge_big_cts, edge_digit_patterns, edge_ksk, edge_mask_values, keyswitch_exact, keyswitch_int)
from exact_pbs import decompose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _accepted_decompositions():
    pairs = set()
    for fname in ("reference_parameter_sets.json", "reference_parameter_sets_compact_pk.json"):
        for r in json.load(open(os.path.join(GOLDEN, fname))).values():
            pairs.add((r["ks_base_log"], r["ks_level"]))
    return sorted(p for p in pairs if 1 <= p[0] <= 7 and p[0] * p[1] <= 62)       # params_supported's range


PAIRS = _accepted_decompositions()


def _toy(bl, L, n=8, N=128, k=1):
    return O.Params(n, k, N, 15, 2, bl, L, 4, 1, 1e-13, 1e-17, f"TOY_KS{L}x{bl}_N{N}_k{k}_n{n}")


def _oracle_keyswitch(p, ksk, cts):
    sk = O.ServerKey.from_keys(p, np.zeros(p.n * p.pbs_level * (p.k + 1) ** 2 * p.N, dtype=np.uint64), ksk, fourier=False)
    return np.stack([sk.keyswitch(c) for c in cts])


def test_the_tables_hold_the_expected_decompositions():
    assert len(PAIRS) == 18 and {b for b, _ in PAIRS} == set(range(1, 8)) and max(L for _, L in PAIRS) == 22


def test_base_log_8_is_refused_with_the_existing_message():
    import fhestr
    ok, why = fhestr.params_supported(fhestr.Params(742, 1, 2048, 23, 1, 8, 2, 4, 4, 7e-6, 3e-16, "KS_8x2"))
    assert not ok and "unsupported keyswitch decomposition (base_log 1..7, base_log * level <= 62)" in why


@pytest.mark.parametrize("bl,L", PAIRS, ids=lambda v: str(v))
def test_integer_decomposer_matches_the_numpy_one_and_recomposes(bl, L):
    rng = np.random.default_rng([bl, L])
    xs = [int(x) for x in rng.integers(0, 2**64, size=200, dtype=np.uint64)] + list(edge_mask_values(bl, L).values())
    vec = decompose(np.array(xs, dtype=np.uint64), bl, L)
    for j, x in enumerate(xs):
        digs = decompose_int(x, bl, L)
        assert digs == [int(v[j]) for v in vec]
        assert all(-(1 << (bl - 1)) <= d <= 1 << (bl - 1) for d in digs)
        rec = sum(d << (64 - bl * (L - it)) for it, d in enumerate(digs)) % 2**64
        assert rec == closest_representable_int(x, bl, L)
        err = (rec - x + 2**63) % 2**64 - 2**63
        assert -(1 << (63 - bl * L)) < err <= 1 << (63 - bl * L)                   # ties round up


@pytest.mark.parametrize("bl,L", PAIRS, ids=lambda v: str(v))
def test_edge_values_are_what_they_claim(bl, L):
    v = edge_mask_values(bl, L)
    h, non_rep = 1 << (bl - 1), 64 - bl * L
    for name, want in edge_digit_patterns(bl, L).items():
        assert decompose_int(v[name], bl, L) == want, name
    assert decompose_int(v["pos_low"], bl, L) == decompose_int(v["pos"], bl, L)
    assert decompose_int(v["neg_max_low"], bl, L) == decompose_int(v["neg_max"], bl, L)
    pos, neg_max = edge_digit_patterns(bl, L)["pos"], edge_digit_patterns(bl, L)["neg_max"]
    assert pos[-1] == h and pos.count(h) == (L + 1) // 2 and (neg_max[0] == -h or L == 1) and neg_max.count(-h) == L // 2
    # no value at all has two neighbouring +B/2 (or -B/2) digits: the patterns above are the extremes that exist
    rng = np.random.default_rng([bl, L, 7])
    for x in rng.integers(0, 2**64, size=300, dtype=np.uint64):
        d = decompose_int(int(x), bl, L)
        assert not any(abs(a) == h and a == b for a, b in zip(d, d[1:]))
    assert decompose_int(v["mid_below"], bl, L) == [0] * L
    assert closest_representable_int(v["mid"], bl, L) == 1 << non_rep == closest_representable_int(v["mid_above"], bl, L)
    step = 1 << non_rep
    assert closest_representable_int(v["hi_mid"], bl, L) - closest_representable_int(v["hi_mid_below"], bl, L) == step
    assert closest_representable_int(v["hi_mid_above"], bl, L) == closest_representable_int(v["hi_mid"], bl, L)
    assert decompose_int(v["carry_top"], bl, L) == [-1] + [0] * (L - 1)            # the carry ran through every level and left
    assert decompose_int(v["round_wrap"], bl, L) == [0] * L and decompose_int(v["ones"], bl, L) == [0] * L
    assert decompose_int(v["below_wrap"], bl, L) == [-1] + [0] * (L - 1)


def test_edge_key_words():
    assert [balanced_digits(w) for w in EDGE_KEY_WORDS[4:]] == [[-128] * 8, [127] * 8, [-128, 127] * 4, [127, -128] * 4]
    for w in EDGE_KEY_WORDS + [0x0123456789ABCDEF, 0x80, 0xFF80]:
        assert sum(s << (8 * t) for t, s in enumerate(balanced_digits(w))) % 2**64 == w
    assert balanced_digits(2**64 - 1) == [-1, 0, 0, 0, 0, 0, 0, 0] and balanced_digits(2**63) == [0] * 7 + [-128]
    p = _toy(3, 5, n=20)
    ksk = edge_ksk(p, np.random.default_rng(1))
    assert ksk.shape == (p.N * 5, 21) and np.array_equal(ksk, edge_ksk(p, np.random.default_rng(1)))        # deterministic
    for j, w in enumerate(EDGE_KEY_WORDS):
        assert (ksk[:, j] == w).all() and (ksk[j % 2::2, 8 + j] == w).all()
    assert (ksk[:, 20] == EDGE_KEY_WORDS[4]).all()


def test_edge_rows():
    p = _toy(3, 5)
    a = edge_big_cts(p, np.random.default_rng(5), 40)
    assert np.array_equal(a, edge_big_cts(p, np.random.default_rng(5), 40)) and a.shape == (40, p.N + 1)
    v = edge_mask_values(3, 5)
    assert set(v.values()) <= set(int(x) for x in a[0, :p.N])                       # every edge value occurs in row 0
    assert {int(x) for x in a[:N_EDGE_ROWS, p.N]} >= {0, 2**63, 2**64 - 1}
    assert (a[1, :p.N] == v["neg_max"]).all() and (a[2, :p.N] == v["pos"]).all() and (a[3, :p.N] == v["neg"]).all()
    for row, pos in ((8, 0), (9, p.N // 6 * 6 - 1), (10, p.N - 1)):
        assert np.flatnonzero(a[row, :p.N]).tolist() == [pos]
    assert len(np.unique(a[N_EDGE_ROWS:], axis=0)) == 40 - N_EDGE_ROWS
    for count in (0, 1, 3, N_EDGE_ROWS):                                           # a smaller batch holds the first rows
        fewer = edge_big_cts(p, np.random.default_rng(5), count)
        assert fewer.shape == (count, p.N + 1) and np.array_equal(fewer[1:, :p.N], a[1:count, :p.N])


@pytest.mark.parametrize("bl,L", PAIRS, ids=lambda v: str(v))
def test_fast_form_equals_the_integer_loop_and_the_oracle(bl, L):
    """Edge rows x edge key and uniform rows x uniform key, both forms and the oracle, word for word."""
    p = _toy(bl, L)
    rng = np.random.default_rng([bl, L, 1])
    cts = edge_big_cts(p, rng, N_EDGE_ROWS + 3)
    for ksk in (edge_ksk(p, rng), rng.integers(0, 2**64, size=(p.N * L, p.n + 1), dtype=np.uint64)):
        fast = keyswitch_exact(p, ksk, cts)
        assert np.array_equal(fast, np.stack([keyswitch_int(p, ksk, c) for c in cts]))
        assert np.array_equal(fast, _oracle_keyswitch(p, ksk, cts))


@pytest.mark.parametrize("p", [_toy(4, 3, n=33, N=128, k=2), _toy(3, 5, n=31, N=256), _toy(7, 2, n=12, N=512), O.TOY_K1, O.TOY_K2],
                         ids=lambda p: p.name)
def test_other_shapes(p):
    rng = np.random.default_rng([p.N, p.k, p.n])
    ksk = edge_ksk(p, rng)
    cts = edge_big_cts(p, rng, N_EDGE_ROWS + 2)
    fast = keyswitch_exact(p, ksk, cts)
    assert np.array_equal(fast[:6], np.stack([keyswitch_int(p, ksk, c) for c in cts[:6]]))
    assert np.array_equal(fast, _oracle_keyswitch(p, ksk, cts))


def test_real_dimensions_against_the_oracle():
    """PARAM_MESSAGE_2_CARRY_2 (10240 x 743 key), more rows than one pass of the digit matrix takes."""
    p = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    rng = np.random.default_rng(22)
    ksk = edge_ksk(p, rng)
    cts = edge_big_cts(p, rng, 515)
    fast = keyswitch_exact(p, ksk, cts)
    pick = [0, 1, 2, 3, 10, 511, 512, 514]
    assert np.array_equal(fast[pick], _oracle_keyswitch(p, ksk, cts[pick]))


def test_the_float64_bound_is_asserted():
    big = O.Params(8, 1, 1 << 29, 15, 2, 7, 8, 4, 1, 1e-13, 1e-17, "TOO_MANY_ROWS")      # 64 * 65535 * 2^32 rows > 2^53
    with pytest.raises(AssertionError, match="2\\^53"):
        ExactKeyswitch(big, np.zeros(0, dtype=np.uint64))
    ok = ExactKeyswitch(O.Params(4, 1, 32768, 15, 2, 7, 8, 16, 16, 1e-13, 1e-17, "N32768_KS8x7"),
                        np.zeros(32768 * 8 * 5, dtype=np.uint64))
    assert ok.bound == 64 * 65535 * 32768 * 8 < 2**53                               # the largest accepted shape: 2^40
