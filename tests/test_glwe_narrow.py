"""Narrow packed GLWE results on the host (csrc/glwe_narrow.cpp, the noise judgement of csrc/client.cpp, the byte form of
csrc/wire_format.cpp) against exact integers written from the definition (tests/exact_narrow.py).  No device is needed.

  test_word_for_word        narrow / widen / extract of the library against the restatement, and the extract against
                            exact_extract.extract_exact of the widened GLWEs, over (N, k) x bits x held x ranges
  test_planted_edge_words   the wrap, the tie and their neighbours at the first and last field of every GLWE and next to
                            every 64-bit boundary of the stream
  test_rounding_error_and_tail_bits  |widen(narrow(x)) - x| <= 2^(63-b) as a wrapped difference; tail bits 0
  test_length, test_refusals, test_wire_round_trip, test_wire_refusals
  test_noise                V_narrow on real keys: variance of the phase difference at b = 12 against (1 + h) / 12 * 2^-2b
  test_model, test_default_bits  fhe_narrow_noise against its definition; the default widths and their refusals
  test_client               pack on the host, narrow, decrypt_narrow"""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_narrow as X
import oracle as O
from conftest import to_fhestr_params
from exact_extract import RANGE_IDS, RANGES, SHAPES, extract_exact


def _f():
    import fhestr
    return fhestr


def _params(N, k):
    return _f().Params(8, k, N, 10, 1, 4, 2, 4, 4, 1e-12, 1e-15, f"NARROW_N{N}_K{k}")


@functools.lru_cache(maxsize=None)
def _glwes(N, k, held):
    rng = np.random.default_rng([N, k, held, 31])
    g = rng.integers(0, 2**64, size=(-(-held // N), k + 1, N), dtype=np.uint64)
    g.setflags(write=False)
    return g


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} of {want.size} words differ from exact; first {bad[:8].tolist()}"


def _ranges(N, held):
    """exact_extract's (first, count), clipped to the blocks the list holds."""
    out = []
    for rng_of, rid in zip(RANGES, RANGE_IDS):
        first, count = rng_of(N)
        first = min(first, held - 1)
        out.append((rid, first, min(count, held - first)))
    return out


def _check_all(N, k, held, b, glwes):
    f, P = _f(), _params(N, k)
    want = X.narrow_exact(glwes, k, N, held, b)
    got = f.glwe_narrow_host(P, glwes, held, b)
    _same(got, want, f"narrow N={N} k={k} held={held} b={b}")
    assert X.tail_bits_zero(got, k, N, held, b)
    wide = X.widen_exact(want, k, N, held, b)
    _same(f.glwe_widen_host(P, want, held, b), wide, f"widen N={N} k={k} held={held} b={b}")
    for rid, first, count in _ranges(N, held):
        rows = f.narrow_sample_extract_host(P, want, held, b, count, first)
        _same(rows, extract_exact(wide, k, N, first, count), f"extract {rid} N={N} k={k} held={held} b={b}")
        _same(rows, f.glwe_sample_extract_host(P, wide, count, first), f"extract {rid} against the library's full-GLWE loop")
    return want, wide


@pytest.mark.parametrize("held_of", X.HELD, ids=X.HELD_IDS)
@pytest.mark.parametrize("b", X.BITS)
@pytest.mark.parametrize("N,k", SHAPES, ids=str)
def test_word_for_word(N, k, b, held_of):
    held = held_of(N)
    _check_all(N, k, held, b, _glwes(N, k, held))


@pytest.mark.parametrize("b", X.BITS)
@pytest.mark.parametrize("N,k", SHAPES, ids=str)
def test_planted_edge_words(N, k, b):
    for w, v in X.edge_words(b):
        assert X.narrow_word(w, b) == v
    held = N + 1
    glwes = X.plant_edges(_glwes(N, k, held), k, N, held, b)
    planted = {w for w, _ in X.edge_words(b)}
    assert planted <= set(glwes.reshape(-1).tolist())
    narrow, wide = _check_all(N, k, held, b, glwes)
    # first field of the list: planted with edge word 0 (2^64 - 1, wraps to 0); the last field of GLWE 0 with edge word 1
    assert int(narrow[0]) & (2**b - 1) == 0 and int(wide[0, 0, 0]) == 0


@pytest.mark.parametrize("b", X.BITS)
def test_rounding_error_and_tail_bits(b):
    N, k, held = 256, 2, 300
    f, P = _f(), _params(N, k)
    glwes = X.plant_edges(_glwes(N, k, held), k, N, held, b)
    narrow = f.glwe_narrow_host(P, glwes, held, b)
    assert X.tail_bits_zero(narrow, k, N, held, b)
    wide = f.glwe_widen_host(P, narrow, held, b).reshape(-1, (k + 1) * N)
    full = glwes.reshape(-1, (k + 1) * N)
    for g in range(2):
        F = k * N + X.blocks_of(N, held, g)
        with np.errstate(over="ignore"):
            d = (wide[g, :F] - full[g, :F]).astype(np.int64)            # the wrapped difference
        assert np.abs(d.astype(object)).max() <= 2**(63 - b)
        assert not wide[g, F:].any()                                    # the coefficients that hold no block
    assert np.array_equal(f.glwe_narrow_host(P, wide, held, b), narrow)  # narrowing what was widened changes nothing


def test_length():
    f = _f()
    for N, k in SHAPES:
        P = _params(N, k)
        for b in X.BITS:
            for held_of in X.HELD:
                held = held_of(N)
                G = -(-held // N)
                want = (G - 1) * -(-(k * N + N) * b // 64) + -(-(k * N + held - (G - 1) * N) * b // 64)
                assert f.narrow_len(P, held, b) == want == X.narrow_len(N, k, held, b)
        assert f.narrow_len(P, N, 7) == 0 and f.narrow_len(P, N, 33) == 0 and f.narrow_len(P, 0, 16) == 0
    P22 = f.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    assert f.narrow_len(P22, 1024, 16) * 8 == 6144 and f.narrow_len(P22, 1024, 13) * 8 == 4992


def test_refusals():
    f = _f()
    L, P = f.lib(), _params(256, 1)
    pc = C.byref(P.c())
    buf = np.zeros(1024, dtype=np.uint64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for call in (lambda: L.fhe_glwe_narrow_host(pc, None, 5, 16, ptr), lambda: L.fhe_glwe_narrow_host(pc, ptr, 5, 16, None),
                 lambda: L.fhe_glwe_widen_host(pc, None, 5, 16, ptr), lambda: L.fhe_glwe_widen_host(None, ptr, 5, 16, ptr),
                 lambda: L.fhe_narrow_sample_extract_host(pc, None, 5, 16, 0, 1, ptr),
                 lambda: L.fhe_narrow_sample_extract_host(pc, ptr, 5, 16, 0, 1, None),
                 lambda: L.fhe_client_decrypt_narrow(None, ptr, 5, 16, ptr),
                 lambda: L.fhe_narrow_noise(pc, None, 16, (C.c_double * 3)()),
                 lambda: L.fhe_narrow_default_bits(pc, C.byref(f._pp((7, 3))), 1, None)):
        assert call() != 0 and b"null pointer" in L.fhe_last_error()
    assert L.fhe_narrow_len(None, 5, 16) == 0
    for bits in (0, 7, 33, 64):
        for call in (lambda: L.fhe_glwe_narrow_host(pc, ptr, 5, bits, ptr), lambda: L.fhe_glwe_widen_host(pc, ptr, 5, bits, ptr),
                     lambda: L.fhe_narrow_sample_extract_host(pc, ptr, 5, bits, 0, 1, ptr),
                     lambda: L.fhe_narrow_noise(pc, C.byref(f._pp((7, 3))), bits, (C.c_double * 3)())):
            assert call() != 0 and b"8 .. 32" in L.fhe_last_error(), bits
        with pytest.raises(f.FheError):
            f.glwe_narrow_host(P, np.zeros((1, 2, 256), dtype=np.uint64), 5, bits)
    narrow = f.glwe_narrow_host(P, _glwes(256, 1, 5), 5, 16)
    for first, count in ((0, 6), (5, 1), (3, 3), (2**32 - 1, 2)):
        assert L.fhe_narrow_sample_extract_host(pc, narrow.ctypes.data_as(C.c_void_p), 5, 16, first, count, ptr) != 0
        assert b"first + count" in L.fhe_last_error()
    assert f.narrow_sample_extract_host(P, narrow, 5, 16, 0, 5).shape == (0, 257)          # count 0 touches nothing
    assert f.narrow_sample_extract_host(P, narrow, 5, 16, 2, 3).shape == (2, 257)
    with pytest.raises(f.FheError, match="narrow list"):
        f.narrow_sample_extract_host(P, narrow[:-1], 5, 16, 1)


def _wire_write(P, narrow, held, bits):
    L = _f().lib()
    n = C.c_size_t()
    assert L.fhe_wire_write_narrow_list(C.byref(P.c()), narrow.ctypes.data_as(C.c_void_p), held, bits, None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, dtype=np.uint8)
    assert L.fhe_wire_write_narrow_list(C.byref(P.c()), narrow.ctypes.data_as(C.c_void_p), held, bits, out.ctypes.data_as(C.c_void_p), n.value - 1,
                                        C.byref(n)) != 0 and b"too small" in L.fhe_last_error()
    assert L.fhe_wire_write_narrow_list(C.byref(P.c()), narrow.ctypes.data_as(C.c_void_p), held, bits, out.ctypes.data_as(C.c_void_p), n.value,
                                        C.byref(n)) == 0 and n.value == out.size
    return out


def _wire_read(P, data, max_held, cap=None, in_len=None):
    """(rc, held, bits, words, consumed); the input is handed over in a buffer of exactly its length."""
    f = _f()
    L = f.lib()
    data = np.array(data, dtype=np.uint8)
    held, bits, used = C.c_uint32(), C.c_uint32(), C.c_size_t()
    args = (C.byref(P.c()), data.ctypes.data_as(C.c_void_p), data.size if in_len is None else in_len)
    if L.fhe_wire_read_narrow_list(*args, None, 0, max_held, C.byref(held), C.byref(bits), C.byref(used)):
        return 1, 0, 0, None, 0
    words = np.zeros(f.narrow_len(P, held.value, bits.value) if cap is None else cap, dtype=np.uint64)
    rc = L.fhe_wire_read_narrow_list(*args, words.ctypes.data_as(C.c_void_p), words.size, max_held, C.byref(held), C.byref(bits), C.byref(used))
    return rc, held.value, bits.value, words, used.value


@pytest.mark.parametrize("b", [8, 13, 32])
@pytest.mark.parametrize("N,k,held", [(256, 1, 1), (256, 2, 257), (512, 3, 512)])
def test_wire_round_trip(N, k, held, b):
    f, P = _f(), _params(N, k)
    narrow = f.glwe_narrow_host(P, _glwes(N, k, held), held, b)
    data = _wire_write(P, narrow, held, b)
    assert data.size == 5 * 8 + narrow.size * 8
    head = data[:40].view("<u8")
    assert head.tolist() == [k, N, b, held, narrow.size] and data[40:].tobytes() == narrow.astype("<u8").tobytes()
    rc, h, bits, words, used = _wire_read(P, data, held)
    assert (rc, h, bits, used) == (0, held, b, data.size) and np.array_equal(words, narrow)
    assert _wire_write(P, words, h, bits).tobytes() == data.tobytes()                      # byte for byte
    # trailing bytes are left alone and not counted
    rc, h, bits, words, used = _wire_read(P, np.concatenate([data, np.full(3, 0xAB, dtype=np.uint8)]), held + 7)
    assert (rc, used) == (0, data.size) and np.array_equal(words, narrow)


def test_wire_refusals():
    f = _f()
    L = f.lib()
    N, k, held, b = 256, 1, 300, 13
    P = _params(N, k)
    narrow = f.glwe_narrow_host(P, _glwes(N, k, held), held, b)
    data = _wire_write(P, narrow, held, b)
    for cut in (0, 7, 8, 31, 32, 39, 40, 41, data.size - 8, data.size - 1):                 # every truncation is refused, none reads past it
        rc, *_ = _wire_read(P, data[:cut].copy(), held)
        assert rc != 0 and b"truncated" in L.fhe_last_error(), cut

    def patched(word, value):
        d = data.copy()
        d[8 * word:8 * word + 8] = np.array([value], dtype="<u8").view(np.uint8)
        return d

    for word, value, reason in ((0, 2, b"parameter set"), (1, 512, b"parameter set"), (2, 7, b"8 .. 32"), (2, 33, b"8 .. 32"), (2, 16, b"words"),
                                (3, held + 1, b"words"), (4, narrow.size - 1, b"words"), (4, 2**61, b"words")):
        rc, *_ = _wire_read(P, patched(word, value), 2**32 - 1)
        assert rc != 0 and reason in L.fhe_last_error(), (word, value, L.fhe_last_error())
    rc, *_ = _wire_read(P, data, held - 1)
    assert rc != 0 and b"the caller accepts" in L.fhe_last_error()
    rc, *_ = _wire_read(P, data, held, cap=narrow.size - 1)
    assert rc != 0 and b"destination" in L.fhe_last_error()
    # a set tail bit, the lowest and the highest (a full stream of (k + 1) N >= 64 fields ends on a word boundary: only the
    # last stream has tail bits)
    used = (k * N + held - N) * b
    assert used % 64
    for bit in (used % 64, 63):
        bad = narrow.copy()
        bad[-1] |= np.uint64(1) << np.uint64(bit)
        d = data.copy()
        d[40:] = bad.astype("<u8").view(np.uint8)
        rc, *_ = _wire_read(P, d, held)
        assert rc != 0 and b"last field" in L.fhe_last_error()
        n = C.c_size_t()
        assert L.fhe_wire_write_narrow_list(C.byref(P.c()), bad.ctypes.data_as(C.c_void_p), held, b, None, 0, C.byref(n)) != 0
    assert L.fhe_wire_write_narrow_list(C.byref(P.c()), None, held, b, None, 0, None) != 0 and b"null pointer" in L.fhe_last_error()
    assert L.fhe_wire_read_narrow_list(C.byref(P.c()), None, 0, None, 0, 1, None, None, None) != 0 and b"null pointer" in L.fhe_last_error()


def test_noise():
    """V_narrow on real keys.  TOY_K1 (N = 256, k = 1): 4,096 encrypted blocks through fhe_packing_keyswitch_host, each
    narrowed to b = 12 and widened again; the sample is the difference of the block's phase, under the client key, between
    the widened and the full GLWE.  Expected variance (1 + h) / 12 * 2^-2b with h the key's actual Hamming weight; tolerance
    5 sqrt(2 / samples) relative -- five standard deviations of a variance estimate from independent samples; the mean is
    zero within five of its own.  Nothing is fitted.
    Every block is packed into a GLWE of its own (held = 1): the coefficients of ONE GLWE share its mask's rounding errors
    -- the half of each sum that the key's mean carries is common to neighbouring coefficients, correlation about
    (1 - 2 |c - c'| / N) / 2 -- so 4,096 coefficients of 16 full GLWEs are worth about 190 independent samples and would not
    support the tolerance; 4,096 masks of their own do."""
    f = _f()
    p = O.TOY_K1
    P = to_fhestr_params(p)
    ck = f.ClientKey(P, 0x5EED0D00)
    pp, key = ck.gen_packing_key((4, 3), seed=17)
    glwe_sk, _ = ck.secret_keys()
    h, b, S = int(glwe_sk.sum()), 12, 4096
    cts = ck.encrypt((np.arange(S) * 5 + 1) % (p.msg_mod * p.carry_mod))
    diff = np.zeros((S, 2, p.N), dtype=np.uint64)
    for j in range(S):
        full = f.packing_keyswitch_host(P, pp, key, cts[j:j + 1])
        narrow = f.glwe_narrow_host(P, full, 1, b)
        with np.errstate(over="ignore"):
            diff[j] = f.glwe_widen_host(P, narrow, 1, b)[0] - full[0]
    # phase at coefficient 0: B[0] - (A[0] s[0] - sum_{i >= 1} A[N - i] s[i])
    s = glwe_sk.astype(np.uint64)
    with np.errstate(over="ignore"):
        a_rev = np.concatenate([diff[:, 0, :1], np.uint64(0) - diff[:, 0, :0:-1]], axis=1)       # A[0], -A[N-1], ..., -A[1]
        ph = diff[:, 1, 0] - (a_rev * s[None, :]).sum(axis=1, dtype=np.uint64)
    err = ph.astype(np.int64).astype(np.float64) / 2.0**64
    want = (1 + h) / 12.0 * 2.0**(-2 * b)
    var, mean = float((err**2).mean()), float(err.mean())
    print(f"narrow noise {p.name} b={b}: key weight {h} of {p.N}, variance {var:.4e}, expected {want:.4e}, ratio {var / want:.4f}; "
          f"mean {mean:.3e}, five deviations {5 * np.sqrt(want / S):.3e}; tolerance {5 * np.sqrt(2 / S):.4f}")
    assert abs(var / want - 1) <= 5 * np.sqrt(2.0 / S)
    assert abs(mean) <= 5 * np.sqrt(want / S)
    ck.close()


def _v_narrow(P, b):
    return (1 + P.k * P.N / 2) / 12 * 2.0**(-2 * b)


@pytest.mark.parametrize("which", ["P22", "TOY_K1"])
def test_model(which):
    f = _f()
    P = f.PARAM_MESSAGE_2_CARRY_2_KS_PBS if which == "P22" else to_fhestr_params(O.TOY_K1)
    for pp in ((7, 3), (7, 2), (4, 3)):
        unpack = f.packing_unpack_noise(P, pp)
        prev = None
        for b in range(8, 33):
            out = f.narrow_noise(P, pp, b)
            want = unpack[0] + _v_narrow(P, b) / f.noise_model(P)["v_pbs"]
            assert abs(out[0] / want - 1) <= 1e-9 and out[1] == unpack[1]
            assert prev is None or (out[0] < prev[0] and out[2] <= prev[2])       # wider is quieter
            prev = out


def _client_target(P):
    """The bound fhe_packing_default_params judges with, recomputed from fhe_noise_model as tests/test_packing_ks.py does:
    the failure probability at the reference-shaped worst case, half a bit of slack, V_pbs times four on unmeasured shapes."""
    import math
    f = _f()
    m = f.noise_model(P)
    safety = 1.0 if f.noise_model_is_calibrated(P) else 4.0
    max_level = (P.msg_mod * P.carry_mod - 1) / max(1, P.msg_mod - 1)
    z = m["half_box"] / math.sqrt(max_level**2 * safety * m["v_pbs"] + m["v_ks"] + m["v_ms"])
    return math.log2(math.erfc(z / math.sqrt(2.0))) + (0.0 if P.grouping == 2 else 0.5)


def test_default_bits():
    """narrow_default_bits returns the smallest admissible width by its own narrow_noise: b passes, b - 1 does not."""
    f = _f()
    P22, TOY = f.PARAM_MESSAGE_2_CARRY_2_KS_PBS, to_fhestr_params(O.TOY_K1)
    for P, pp in ((P22, (7, 3)), (P22, (7, 2)), (TOY, (7, 2)), (TOY, (4, 3))):
        target = _client_target(P)
        passes = {True: lambda o: o[0] <= o[1], False: lambda o: o[2] <= target}
        for operand in (True, False):
            widths = [b for b in range(8, 33) if passes[operand](f.narrow_noise(P, pp, b))]
            if not widths:
                with pytest.raises(f.FheError, match=rf"\({pp[0]}, {pp[1]}\)"):
                    f.narrow_default_bits(P, pp, operand)
                continue
            b = f.narrow_default_bits(P, pp, operand)
            print(f"narrow default {P.name} pp={pp} {'operand' if operand else 'client'}: {b} bits, narrow_noise {f.narrow_noise(P, pp, b)}, "
                  f"one below {f.narrow_noise(P, pp, max(8, b - 1))}, client bound 2^{target:.2f}")
            assert b == widths[0] and widths == list(range(b, 33))
    assert f.narrow_default_bits(P22, (7, 3), True) == 16 and f.narrow_default_bits(P22, (7, 3), False) == 13
    assert f.narrow_default_bits(P22, (7, 2), False) == 13
    nominal, budget, _ = f.narrow_noise(P22, (7, 3), 16)
    assert abs(nominal - 36.3) < 0.1 and abs(budget - 138.2) < 0.1
    below = f.narrow_noise(P22, (7, 3), 15)
    assert below[0] > below[1]                                # refused as an operand one bit below the default
    with pytest.raises(f.FheError, match=r"\(7, 2\)"):       # the packing alone is above the budget: refused outright
        f.narrow_default_bits(P22, (7, 2), True)
    assert f.packing_unpack_noise(P22, (7, 2))[0] > budget


@pytest.mark.parametrize("count", [1, 256, 300])
def test_client(count):
    f = _f()
    p = O.TOY_K1
    P = to_fhestr_params(p)
    ck = f.ClientKey(P, 0x5EED0D10)
    pp, key = ck.gen_packing_key(seed=19)
    msgs = (np.arange(count) * 7 + 3) % (p.msg_mod * p.carry_mod)
    glwes = f.packing_keyswitch_host(P, pp, key, ck.encrypt(msgs))
    for b in (f.narrow_default_bits(P, pp, operand=False), 32):
        narrow = f.glwe_narrow_host(P, glwes, count, b)
        assert np.array_equal(ck.decrypt_narrow(narrow, count, b), msgs)
        ns = f.NarrowString(narrow, count, count // f.blocks_per_char(P), b)
        assert ns.shape == (1, narrow.size) and (ns.count, ns.bits) == (count, b) and ns[0].bits == b
        assert np.array_equal(ck.decrypt_narrow(ns), msgs)
        assert f.EncryptedCount(ns, params=P).n_max == P.msg_mod**count - 1 if count == 1 else True   # its digits are counted like a PackedString's
        assert np.array_equal(ck.decrypt_packed(f.glwe_widen_host(P, narrow, count, b), count), msgs)
        with pytest.raises(f.FheError):
            ck.decrypt_narrow(narrow[:-1], count, b)
    ck.close()
