"""Packed GLWE ciphertexts as inputs on the GPU (csrc/glwe_extract_kernels.hip.h, Packing::unpack_dev) against exact
integers (tests/exact_extract.py).  Every raw comparison is equality of all words; every check reads
fhe_engine_unpack_info, so a host fallback could not pass.

  test_raw_extract          (N, k) x (first, count) of exact_extract: the host-array entry point and the _dev form, the
                            latter into a 16-byte aligned buffer and into one off by 8 bytes (both row parities first)
  test_k2_n256_has_no_engine  (256, 2) of the CPU grid: the library instantiates no blind rotation for it, no engine can be
                            created, so the device kernel cannot be reached; k = 2 runs at N = 128 and N = 1024 instead
  test_rows_spanning_workgroups  (8192, 1), count 3: two workgroups per row
  test_pack_then_unpack_raw toy set and PARAM_MESSAGE_2_CARRY_2, 64 blocks: decrypts to the inputs
  test_raw_noise            2,048 device-packed PBS outputs of PARAM_MESSAGE_2_CARRY_2, unpacked raw: phase-error variance
                            within 15 % of fhe_packing_unpack_noise's out[0] * V_pbs
  test_refresh              refreshed blocks decrypt to the inputs, a second PBS on them stays within the parity tests'
                            8 sigma; the refusals (no packing key; a decomposition the model puts above the budget)
  test_refresh_index_array_grows  refreshes of 3, 40, 3 blocks on one engine: the table-index array is allocated, grown, reused
  test_end_to_end_p22       contains(to_upper(hay, packed=True), pat) with the packed result passed straight back in,
                            op_many over packed rows, packed=True on a packed operand"""
import functools

import numpy as np
import pytest

import oracle as O
from exact_extract import RANGE_IDS, RANGES, SHAPES, extract_exact, random_glwes

pytestmark = pytest.mark.gpu

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
# engines exist only for shapes with a blind-rotation kernel: the level count is the one the library instantiates per (N, k)
LEVELS = {(256, 1): 2, (512, 3): 1, (2048, 1): 1, (128, 2): 1, (1024, 2): 1, (8192, 1): 1}
GPU_SHAPES = [s for s in SHAPES if s != (256, 2)] + [(128, 2), (1024, 2)]
# the refresh twin: PARAM_MESSAGE_2_CARRY_2's GLWE side with n = 16; its default pair (7, 3) is admitted
TWIN = O.Params(16, 1, 2048, 23, 1, 3, 5, 4, 4, 1e-13, 1e-17, "TOY_N2048_K1_n16")


def _fp(p):
    import fhestr
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name)


def _shape_params(N, k):
    import fhestr
    return fhestr.Params(8, k, N, 10, LEVELS[(N, k)], 4, 2, 4, 4, 1e-12, 1e-15, f"EXTRACT_N{N}_K{k}")


_ENGINES = {}


def _engine(N, k):
    import fhestr
    if (N, k) not in _ENGINES:
        _ENGINES[(N, k)] = fhestr.Engine(_shape_params(N, k), 0)
        assert not _ENGINES[(N, k)].unpack_info()["ran"]
    return _ENGINES[(N, k)]


@functools.lru_cache(maxsize=None)
def _case(N, k, first, count):
    glwes = random_glwes(k, N, first, count, 9)
    want = extract_exact(glwes, k, N, first, count)
    glwes.setflags(write=False)
    want.setflags(write=False)
    return glwes, want


def _assert_words(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad):
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ from exact; first (row, word) {bad[:12].tolist()}; "
                             f"rows {np.unique(bad[:, 0])[:16].tolist()}, words {np.unique(bad[:, 1])[:16].tolist()}")


def _workgroups(N, k, count):
    return count * -(-(k * N // 2) // 2048)


def _check_raw(N, k, first, count):
    import torch
    eng = _engine(N, k)
    glwes, want = _case(N, k, first, count)
    big = k * N + 1
    got = eng.unpack(glwes, count, first=first, refresh=False)
    info = eng.unpack_info()
    assert info == {"ran": True, "rows": count, "workgroups": _workgroups(N, k, count), "refreshed": False}, info
    _assert_words(got, want, f"host entry N={N} k={k} first={first} count={count}")
    d_glwes = torch.from_numpy(glwes.view(np.int64).copy()).cuda()       # the cached case is read-only
    for off in (0, 1):
        d = torch.full((count * big + 2,), -1, dtype=torch.int64, device="cuda")
        assert d.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        assert eng.unpack(d_in=d_glwes.data_ptr(), count=count, first=first, refresh=False, d_out=d.data_ptr() + 8 * off) is None
        info = eng.unpack_info()
        eng.synchronize()
        assert (info["ran"], info["rows"], info["refreshed"]) == (True, count, False)
        h = d.cpu().numpy().view(np.uint64)
        _assert_words(h[off:off + count * big].reshape(count, big), want, f"_dev N={N} k={k} first={first} count={count} offset {8 * off}")
        guard = np.delete(h, np.s_[off:off + count * big])
        assert (guard == 2**64 - 1).all(), f"offset {8 * off}: words outside the output were written"


@pytest.mark.parametrize("rng_of", RANGES, ids=RANGE_IDS)
@pytest.mark.parametrize("N,k", GPU_SHAPES, ids=lambda v: str(v))
def test_raw_extract(N, k, rng_of):
    _check_raw(N, k, *rng_of(N))


def test_k2_n256_has_no_engine():
    import fhestr
    for level in (1, 2, 3):
        with pytest.raises(fhestr.FheError, match="no blind-rotation kernel"):
            fhestr.Engine(fhestr.Params(8, 2, 256, 10, level, 4, 2, 4, 4, 1e-12, 1e-15, "EXTRACT_N256_K2"), 0)


def test_rows_spanning_workgroups():
    _check_raw(8192, 1, 8190, 3)                            # the last two rows of one GLWE and the first of the next
    assert _engine(8192, 1).unpack_info()["workgroups"] == 6


def test_zero_count_is_a_no_op():
    eng = _engine(256, 1)
    before = eng.unpack_info()
    out = eng.unpack(np.zeros((1, 2, 256), dtype=np.uint64), 0, refresh=False)
    assert out.shape == (0, 257) and eng.unpack_info() == before
    import fhestr
    assert fhestr.lib().fhe_engine_unpack_glwes_dev(eng.handle, None, 0, 0, 1, None) == 0
    assert fhestr.lib().fhe_engine_unpack_glwes_dev(eng.handle, None, 0, 1, 0, None) == 1
    assert "null pointer" in fhestr.lib().fhe_last_error().decode()


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    for rig in _RIGS.values():
        rig.eng.close()
        rig.ck.close()
    _RIGS.clear()


# ---- with real keys -----------------------------------------------------------------------------------------------------

class _Rig:
    def __init__(self, p, seed, server_keys=True):
        import fhestr
        self.P = _fp(p)
        self.ck = fhestr.ClientKey(self.P, seed)
        self.eng = fhestr.Engine(self.P, 0)
        self.glwe_sk, small_sk = self.ck.secret_keys()
        if server_keys:
            self.eng.generate_keys(self.glwe_sk, small_sk, seed + 1)
        self.pp = None

    def packing_key(self, pp=None):
        if pp is None or pp != self.pp:
            self.pp, key = self.ck.gen_packing_key(pp, seed=0x5EED0C10)
            self.eng.load_packing_key(self.pp, key)
        return self.pp

    def phase_errors(self, cts, msgs):
        """(phase - message * delta) / 2^64 of big-key LWEs, signed."""
        cts = np.asarray(cts, dtype=np.uint64)
        delta = np.uint64(2**63 // (self.P.msg_mod * self.P.carry_mod))
        with np.errstate(over="ignore"):
            ph = cts[:, -1] - cts[:, :-1][:, self.glwe_sk.astype(bool)].sum(axis=1, dtype=np.uint64)
            err = ph - np.asarray(msgs, dtype=np.uint64) * delta
        return err.astype(np.int64).astype(np.float64) / 2.0**64


_RIGS = {}


def _rig(p, seed, server_keys=True):
    if p.name not in _RIGS:
        _RIGS[p.name] = _Rig(p, seed, server_keys)
    return _RIGS[p.name]


@pytest.mark.parametrize("p", [O.TOY_K1, P22], ids=lambda p: p.name)
def test_pack_then_unpack_raw(p):
    rig = _rig(p, 0x5EED0C00 + p.N)
    rig.packing_key()
    M = p.msg_mod * p.carry_mod
    msgs = (np.arange(64) * 7 + 3) % M
    glwes = rig.eng.pack(rig.ck.encrypt(msgs))
    lwes = rig.eng.unpack(glwes, 64, refresh=False)
    assert rig.eng.unpack_info() == {"ran": True, "rows": 64, "workgroups": 64, "refreshed": False}
    assert np.array_equal(rig.ck.decrypt(lwes), msgs)
    import fhestr
    _assert_words(lwes, fhestr.glwe_sample_extract_host(rig.P, glwes, 64), "device against the host loop")
    tail = rig.eng.unpack(glwes, 10, first=54, refresh=False)
    _assert_words(tail, lwes[54:], "first = 54")


def test_raw_noise():
    """One full GLWE of PARAM_MESSAGE_2_CARRY_2: 2,048 PBS outputs of known messages, packed on the device with the default
    pair, extracted raw.  Model: out[0] * V_pbs = V_pbs + packing variance (here almost all of it the rounding of the mask
    to 2^-14 against about k N / 2 key bits).  Band: +-15 %, the one tests/test_compact_pk.py uses; 2,048 samples give a
    relative standard deviation of 3 %."""
    import fhestr
    import torch
    rig = _rig(P22, 0x5EED0C00 + P22.N)
    pp = rig.packing_key()
    assert pp == fhestr.packing_default_params(rig.P) == (7, 2)
    P, eng = rig.P, rig.eng
    M, B = P.msg_mod * P.carry_mod, P.N
    msgs = (np.arange(B) * 5 + 1) % M
    lut_id, _ = eng.generate_lookup_table(lambda x: x)
    d_in = torch.from_numpy(rig.ck.encrypt(msgs).view(np.int64)).cuda()
    d_idx = torch.full((B,), lut_id, dtype=torch.int32).cuda()
    d_mid = torch.zeros_like(d_in)
    d_glwe = torch.zeros((1, P.k + 1, P.N), dtype=torch.int64).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_mid.data_ptr(), B)
    eng.pack(d_in=d_mid.data_ptr(), count=B, d_out=d_glwe.data_ptr())
    eng.unpack(d_in=d_glwe.data_ptr(), count=B, refresh=False, d_out=d_out.data_ptr())
    eng.synchronize()
    assert eng.unpack_info() == {"ran": True, "rows": B, "workgroups": B, "refreshed": False}
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(rig.ck.decrypt(raw), msgs)
    err = rig.phase_errors(raw, msgs)
    pbs = rig.phase_errors(d_mid.cpu().numpy().view(np.uint64), msgs)
    nominal, _ = fhestr.packing_unpack_noise(P, pp)
    model = nominal * fhestr.noise_model(P)["v_pbs"]
    print(f"raw unpack noise {P.name} pp={pp}: variance {err.var():.4e} (mean {err.mean():.2e}), model {model:.4e} = {nominal:.1f} nominal, "
          f"ratio {err.var() / model:.4f}; PBS outputs alone {pbs.var():.4e}, V_pbs {fhestr.noise_model(P)['v_pbs']:.4e}; "
          f"key weight {int(rig.glwe_sk.sum())} of {P.k * P.N}")
    assert abs(err.var() / model - 1) <= 0.15


def test_refresh():
    import fhestr
    rig = _rig(TWIN, 0x5EED0C40)
    P, eng, ck = rig.P, rig.eng, rig.ck
    # no packing key yet: the raw form works, the refresh is refused
    glwe0 = np.zeros((1, P.k + 1, P.N), dtype=np.uint64)
    assert eng.unpack(glwe0, 3, refresh=False).shape == (3, P.big_size)
    with pytest.raises(fhestr.FheError, match="packing key"):
        eng.unpack(glwe0, 3, refresh=True)
    pp = rig.packing_key()
    nominal, budget = fhestr.packing_unpack_noise(P, pp)
    assert nominal <= budget
    M, B = P.msg_mod * P.carry_mod, 70
    msgs = (np.arange(B) * 3 + 2) % M
    glwes = eng.pack(ck.encrypt(msgs))
    fresh = eng.unpack(glwes, B)                            # refresh=True is the default
    assert eng.unpack_info() == {"ran": True, "rows": B, "workgroups": B, "refreshed": True}
    assert np.array_equal(ck.decrypt(fresh), msgs)
    raw = eng.unpack(glwes, B, refresh=False)
    assert not np.array_equal(raw, fresh)
    f = lambda x: (5 * x + 3) % M
    lut_id, _ = eng.generate_lookup_table(f)
    again = eng.apply_lookup_table(fresh, np.full(B, lut_id, dtype=np.uint32))
    want = np.array([f(int(m)) for m in msgs])
    assert np.array_equal(ck.decrypt(again), want)
    tol = 8.0 * np.sqrt(2.0 * fhestr.noise_model(P)["v_pbs"])
    e1, e2 = np.abs(rig.phase_errors(fresh, msgs)).max(), np.abs(rig.phase_errors(again, want)).max()
    print(f"refresh {P.name} pp={pp}: raw block {nominal:.2f} nominal (budget {budget:.1f}); max phase error after the refresh {e1:.3e}, "
          f"after a second PBS {e2:.3e}, 8 sigma {tol:.3e}")
    assert e1 <= tol and e2 <= tol


def test_refresh_index_array_grows():
    """The refresh keeps one table index per block of its largest batch so far.  An engine of its own: the shared twin's
    first refresh already has 70 blocks."""
    rig = _Rig(TWIN, 0x5EED0C60)
    try:
        P, eng, ck = rig.P, rig.eng, rig.ck
        rig.packing_key()
        msgs = (np.arange(40) * 3 + 2) % (P.msg_mod * P.carry_mod)
        glwes = eng.pack(ck.encrypt(msgs))
        for count in (3, 40, 3):
            fresh = eng.unpack(glwes, count)
            assert eng.unpack_info() == {"ran": True, "rows": count, "workgroups": _workgroups(P.N, P.k, count), "refreshed": True}
            assert np.array_equal(ck.decrypt(fresh), msgs[:count])
    finally:
        rig.eng.close()
        rig.ck.close()


def test_refresh_refused_above_the_budget():
    """TOY_K1 with its default pair (7, 2): 509 nominal variances against a budget of 99.6 (tests/test_glwe_extract.py)."""
    import fhestr
    rig = _rig(O.TOY_K1, 0x5EED0C00 + O.TOY_K1.N)
    pp = rig.packing_key()
    nominal, budget = fhestr.packing_unpack_noise(rig.P, pp)
    assert nominal > budget
    glwes = rig.eng.pack(rig.ck.encrypt(np.arange(8) % 16))
    before = rig.eng.unpack_info()
    with pytest.raises(fhestr.FheError, match="refresh refused"):
        rig.eng.unpack(glwes, 8, refresh=True)
    assert rig.eng.unpack_info() == before                  # refused before anything was launched
    assert np.array_equal(rig.ck.decrypt(rig.eng.unpack(glwes, 8, refresh=False)), np.arange(8) % 16)


def test_end_to_end_p22():
    """PARAM_MESSAGE_2_CARRY_2, capacity 8, packing pair (7, 3): the default (7, 2) is refused for the refresh on this set
    (564 nominal variances against a budget of 138), the third level brings a raw block to 1.03."""
    import fhestr
    rig = _rig(P22, 0x5EED0C00 + P22.N)
    pp = rig.packing_key((7, 3))
    nominal, budget = fhestr.packing_unpack_noise(rig.P, pp)
    assert nominal <= budget
    P, eng, ck = rig.P, rig.eng, rig.ck
    ops = fhestr.FheStringOps(eng)
    cap = 8
    n_blocks = cap * ops.bpc
    enc = lambda t, c=cap: ck.encrypt(fhestr.string_to_blocks(P, t, c))
    hay, other = b"a Fox", b"b dog"
    up = ops.to_upper(enc(hay), packed=True)
    assert isinstance(up, fhestr.PackedString) and (up.count, up.capacity) == (n_blocks, cap) and up.shape == (1, P.k + 1, P.N)
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(up, n_blocks)) == hay.upper()
    up_expanded = ops.to_upper(enc(hay))
    for pat in (b"FOX", b"Fox"):
        got = ops.contains(up, enc(pat, 4))                 # the packed result straight back in
        info = eng.unpack_info()
        assert info == {"ran": True, "rows": n_blocks, "workgroups": n_blocks, "refreshed": True}, info
        assert ck.decrypt(got.reshape(1, -1))[0] == ck.decrypt(ops.contains(up_expanded, enc(pat, 4)).reshape(1, -1))[0] == int(pat in hay.upper())
        assert ck.decrypt(ops.contains(up, pat).reshape(1, -1))[0] == int(pat in hay.upper())       # clear pattern
    # packed in, packed out: only GLWEs cross PCIe
    low = ops.to_lower(up, packed=True)
    assert isinstance(low, fhestr.PackedString) and low.count == n_blocks
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(low, n_blocks)) == hay.lower()
    flag = ops.contains(up, enc(b"FOX", 4), packed=True)
    assert flag.shape == (P.k + 1, P.N) and ck.decrypt_packed(flag, 1)[0] == 1
    # a packed second operand
    assert ck.decrypt(ops.eq(enc(hay.upper()), up).reshape(1, -1))[0] == 1
    # op_many over two packed rows agrees with the single runs
    up2 = ops.to_upper(enc(other), packed=True)
    many = ops.op_many("contains", [up, up2], enc(b"FOX", 4))
    assert many.shape == (2, 1, P.big_size)
    singles = [ck.decrypt(ops.contains(x, enc(b"FOX", 4)).reshape(1, -1))[0] for x in (up, up2)]
    assert ck.decrypt(many[:, 0]).tolist() == singles == [1, 0]
    many_packed = ops.op_many("to_lower", [up, up2], packed=True)
    dec = ck.decrypt_packed(many_packed, 2 * n_blocks)
    assert [fhestr.blocks_to_string(P, dec[:n_blocks]), fhestr.blocks_to_string(P, dec[n_blocks:])] == [hay.lower(), other.lower()]
    ops.close()
