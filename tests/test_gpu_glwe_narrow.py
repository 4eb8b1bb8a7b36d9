"""Narrow packed GLWE results on the GPU (csrc/glwe_narrow_kernels.hip.h, Packing::narrow_dev / unpack_narrow_dev)
against exact integers (tests/exact_narrow.py, tests/exact_extract.py).  Every raw comparison is equality of all words;
every check reads fhe_engine_narrow_info, so a host fallback could not pass.

  test_narrow_on_device     (N, k) x bits x held: the host-array entry and the _dev form, the latter between guard words
  test_extract_from_narrow  the same shapes and bits, planted edge words, the ranges of exact_extract clipped to held: the
                            host entry and _dev into a 16-byte aligned buffer and one off by 8 bytes, with guards
  test_rows_spanning_workgroups  (8192, 1), 3 rows: two workgroups per row
  test_zero_count_is_a_no_op
  test_shared_staging_across_families  one engine in throughput mode 2, host arrays: unpack, unpack_narrow, a larger unpack, narrow --
                            the staging buffers the two families share are grown by one after the other used them
  test_pack_narrow_unpack_raw  toy twin and PARAM_MESSAGE_2_CARRY_2, 64 blocks: pack -> narrow on the device -> raw unpack decrypts
  test_refresh, test_refresh_refusals
  test_raw_noise            2,048 device-packed PBS outputs, narrowed at the operand-grade default, unpacked raw: phase-error
                            variance within 15 % of narrow_noise's out[0] * V_pbs (the narrowing's term dominates)
  test_string_operations_p22   packed=Narrow() through FheStringOps: results go back in as operands"""
import functools

import numpy as np
import pytest

import exact_narrow as X
import oracle as O
from exact_extract import RANGE_IDS, RANGES, extract_exact

pytestmark = pytest.mark.gpu

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
LEVELS = {(256, 1): 2, (128, 2): 1, (512, 3): 1, (2048, 1): 1, (8192, 1): 1}     # the level count the library instantiates per (N, k)
GPU_SHAPES = [(256, 1), (128, 2), (512, 3), (2048, 1)]
GPU_BITS = [8, 13, 16, 31, 32]
TWIN = O.Params(16, 1, 2048, 23, 1, 3, 5, 4, 4, 1e-13, 1e-17, "TOY_N2048_K1_n16")   # PARAM_MESSAGE_2_CARRY_2's GLWE side with n = 16
GUARD = 2**64 - 1


def _fp(p):
    import fhestr
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name)


_ENGINES, _RIGS = {}, {}


def _engine(N, k):
    import fhestr
    if (N, k) not in _ENGINES:
        _ENGINES[(N, k)] = fhestr.Engine(fhestr.Params(8, k, N, 10, LEVELS[(N, k)], 4, 2, 4, 4, 1e-12, 1e-15, f"NARROW_N{N}_K{k}"), 0)
        assert not _ENGINES[(N, k)].narrow_info()["ran"]
    return _ENGINES[(N, k)]


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


@functools.lru_cache(maxsize=None)
def _case(N, k, held, b):
    """Random GLWEs with the edge words planted, their narrow list and the widened GLWEs, all exact and read-only."""
    rng = np.random.default_rng([N, k, held, b, 77])
    glwes = rng.integers(0, 2**64, size=(-(-held // N), k + 1, N), dtype=np.uint64)
    glwes = X.plant_edges(glwes, k, N, held, b)
    narrow = X.narrow_exact(glwes, k, N, held, b)
    wide = X.widen_exact(narrow, k, N, held, b)
    for a in (glwes, narrow, wide):
        a.setflags(write=False)
    return glwes, narrow, wide


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} of {want.size} words differ from exact; first {bad[:12].tolist()}"


def _guarded(n_words, lead):
    """A device buffer of `lead` guard words, n_words payload words and 2 more guard words; 16-byte aligned."""
    import torch
    d = torch.full((lead + n_words + 2,), -1, dtype=torch.int64, device="cuda")
    assert d.data_ptr() % 16 == 0
    return d


def _payload(d, n_words, lead, what):
    h = d.cpu().numpy().view(np.uint64)
    assert (np.delete(h, np.s_[lead:lead + n_words]) == GUARD).all(), f"{what}: words outside the output were written"
    return h[lead:lead + n_words]


@pytest.mark.parametrize("b", GPU_BITS)
@pytest.mark.parametrize("N,k", GPU_SHAPES, ids=str)
def test_narrow_on_device(N, k, b):
    import torch
    eng = _engine(N, k)
    for held in (1, N, 2 * N + 1):
        glwes, want, _ = _case(N, k, held, b)
        wgs = -(-want.size // 256)
        got = eng.narrow(glwes, held, b)
        assert eng.narrow_info() == {"ran": True, "kernel": "narrow", "items": want.size, "workgroups": wgs, "bits": b}
        assert (got.count, got.bits, got.shape) == (held, b, (1, want.size))
        _same(np.asarray(got).reshape(-1), want, f"host entry N={N} k={k} held={held} b={b}")
        assert X.tail_bits_zero(np.asarray(got), k, N, held, b)
        d_glwes = torch.from_numpy(glwes.view(np.int64).copy()).cuda()
        d = _guarded(want.size, 2)
        torch.cuda.synchronize()
        assert eng.narrow(d_in=d_glwes.data_ptr(), held=held, bits=b, d_out=d.data_ptr() + 16) is None
        info = eng.narrow_info()
        eng.synchronize()
        assert info == {"ran": True, "kernel": "narrow", "items": want.size, "workgroups": wgs, "bits": b}
        _same(_payload(d, want.size, 2, "_dev narrow"), want, f"_dev N={N} k={k} held={held} b={b}")


@pytest.mark.parametrize("b", [13, 32])
@pytest.mark.parametrize("N,k", [(128, 2), (2048, 1)], ids=str)
def test_widen_on_device(N, k, b):
    """The way back on the device, the first step of the two-step route scripts/glwe_narrow_timing.py times."""
    import torch
    eng = _engine(N, k)
    for held in (1, 2 * N + 1):
        _, narrow, wide = _case(N, k, held, b)
        d_narrow = torch.from_numpy(narrow.view(np.int64).copy()).cuda()
        d = _guarded(wide.size, 2)
        torch.cuda.synchronize()
        eng.widen(d_narrow.data_ptr(), held, b, d.data_ptr() + 16)
        info = eng.narrow_info()
        eng.synchronize()
        assert info == {"ran": True, "kernel": "widen", "items": wide.size, "workgroups": -(-wide.size // 256), "bits": b}
        _same(_payload(d, wide.size, 2, "_dev widen"), wide.reshape(-1), f"widen N={N} k={k} held={held} b={b}")


def _workgroups(N, k, count):
    return count * -(-(k * N // 2) // 2048)


def _check_extract(N, k, held, b, first, count):
    import torch
    eng = _engine(N, k)
    _, narrow, wide = _case(N, k, held, b)
    want = extract_exact(wide, k, N, first, count)
    big = k * N + 1
    info_want = {"ran": True, "kernel": "extract", "items": count, "workgroups": _workgroups(N, k, count), "bits": b}
    got = eng.unpack_narrow(narrow, held, b, count=count, first=first, refresh=False)
    assert eng.narrow_info() == info_want
    _same(got, want, f"host entry N={N} k={k} held={held} b={b} first={first} count={count}")
    d_narrow = torch.from_numpy(narrow.view(np.int64).copy()).cuda()
    for off in (0, 1):                                       # both row parities first
        d = _guarded(count * big, 2 + off)
        torch.cuda.synchronize()
        assert eng.unpack_narrow(d_in=d_narrow.data_ptr(), held=held, bits=b, count=count, first=first, refresh=False,
                                 d_out=d.data_ptr() + 8 * (2 + off)) is None
        info = eng.narrow_info()
        eng.synchronize()
        assert info == info_want
        _same(_payload(d, count * big, 2 + off, "_dev extract").reshape(count, big), want,
              f"_dev N={N} k={k} held={held} b={b} first={first} count={count} offset {8 * off}")


@pytest.mark.parametrize("b", GPU_BITS)
@pytest.mark.parametrize("N,k", GPU_SHAPES, ids=str)
def test_extract_from_narrow(N, k, b):
    before = _engine(N, k).unpack_info()
    for held in (N + 1, 2 * N + 1):                          # a last stream of one block; every range unclipped
        for rng_of, rid in zip(RANGES, RANGE_IDS):
            first, count = rng_of(N)
            first = min(first, held - 1)
            count = min(count, held - first)
            if held == N + 1 and rid not in ("cross", "unaligned"):   # the others read the same fields as with 2N + 1 held
                continue
            _check_extract(N, k, held, b, first, count)
    assert _engine(N, k).unpack_info() == before            # the full-GLWE form's record is its own


def test_rows_spanning_workgroups():
    _check_extract(8192, 1, 8193, 13, 8190, 3)               # the last two rows of one GLWE and the one block of the next
    assert _engine(8192, 1).narrow_info()["workgroups"] == 6


def test_zero_count_is_a_no_op():
    import fhestr
    eng = _engine(256, 1)
    _, narrow, _ = _case(256, 1, 257, 13)
    eng.unpack_narrow(narrow, 257, 13, count=1, refresh=False)
    before = eng.narrow_info()
    assert eng.unpack_narrow(narrow, 257, 13, count=0, first=5, refresh=False).shape == (0, 257) and eng.narrow_info() == before
    L = fhestr.lib()
    assert L.fhe_engine_unpack_narrow_dev(eng.handle, None, 257, 13, 0, 0, 1, None) == 0
    assert L.fhe_engine_narrow_glwes_dev(eng.handle, None, 0, 13, None) == 0 and eng.narrow_info() == before
    assert L.fhe_engine_unpack_narrow_dev(eng.handle, None, 257, 13, 0, 1, 0, None) == 1 and b"null pointer" in L.fhe_last_error()
    with pytest.raises(fhestr.FheError, match="holds 257"):
        eng.unpack_narrow(narrow, 257, 13, count=2, first=256, refresh=False)
    with pytest.raises(fhestr.FheError, match="8 .. 32"):
        eng.narrow(np.zeros((1, 2, 256), dtype=np.uint64), 5, 7)
    assert eng.narrow_info() == before


def test_shared_staging_across_families():
    """The host forms stage through buffers two families share: the extracted rows of unpack and unpack_narrow leave through
    one, the GLWEs of narrow and the list of unpack_narrow enter through another.  Each is used by one family, then by the
    other, then grown by the first, under throughput mode 2 (a growth waits for every stream); every result is exact."""
    import fhestr
    N, k = min(s for s in GPU_SHAPES if s[1] == 1)
    held = 2 * N + 3
    glwes, narrow, wide = _case(N, k, held, 16)
    eng = fhestr.Engine(fhestr.Params(8, k, N, 10, LEVELS[(N, k)], 4, 2, 4, 4, 1e-12, 1e-15, f"NARROW_N{N}_K{k}"), 0)
    try:
        eng.set_pipeline(2)
        unpacked = lambda count: {"ran": True, "rows": count, "workgroups": _workgroups(N, k, count), "refreshed": False}
        _same(eng.unpack(glwes, 5, first=N + 1, refresh=False), extract_exact(glwes, k, N, N + 1, 5), "unpack of 5")
        assert eng.unpack_info() == unpacked(5) and not eng.narrow_info()["ran"]
        _same(eng.unpack_narrow(narrow, held, 16, count=7, first=N - 2, refresh=False), extract_exact(wide, k, N, N - 2, 7), "unpack_narrow of 7")
        assert eng.narrow_info() == {"ran": True, "kernel": "extract", "items": 7, "workgroups": _workgroups(N, k, 7), "bits": 16}
        assert eng.unpack_info() == unpacked(5)
        _same(eng.unpack(glwes, N + 9, first=N + 1, refresh=False), extract_exact(glwes, k, N, N + 1, N + 9), f"unpack of {N + 9}")
        assert eng.unpack_info() == unpacked(N + 9)
        got = eng.narrow(glwes, held, 16)
        _same(np.asarray(got).reshape(-1), narrow, f"narrow of {held}")
        assert eng.narrow_info() == {"ran": True, "kernel": "narrow", "items": narrow.size, "workgroups": -(-narrow.size // 256), "bits": 16}
    finally:
        eng.close()


# ---- with real keys -----------------------------------------------------------------------------------------------------

class _Rig:
    def __init__(self, p, seed):
        import fhestr
        self.P = _fp(p)
        self.ck = fhestr.ClientKey(self.P, seed)
        self.eng = fhestr.Engine(self.P, 0)
        self.glwe_sk, small_sk = self.ck.secret_keys()
        self.eng.generate_keys(self.glwe_sk, small_sk, seed + 1)
        self.pp, self.key = self.ck.gen_packing_key((7, 3), seed=0x5EED0E10)

    def load(self):
        self.eng.load_packing_key(self.pp, self.key)

    def phase_errors(self, cts, msgs):
        """(phase - message * delta) / 2^64 of big-key LWEs, signed."""
        cts = np.asarray(cts, dtype=np.uint64)
        delta = np.uint64(2**63 // (self.P.msg_mod * self.P.carry_mod))
        with np.errstate(over="ignore"):
            ph = cts[:, -1] - cts[:, :-1][:, self.glwe_sk.astype(bool)].sum(axis=1, dtype=np.uint64)
            err = ph - np.asarray(msgs, dtype=np.uint64) * delta
        return err.astype(np.int64).astype(np.float64) / 2.0**64


def _rig(p):
    if p.name not in _RIGS:
        _RIGS[p.name] = _Rig(p, 0x5EED0E00 + p.n)
    _RIGS[p.name].load()
    return _RIGS[p.name]


@pytest.mark.parametrize("p", [TWIN, P22], ids=lambda p: p.name)
def test_pack_narrow_unpack_raw(p):
    import fhestr
    import torch
    rig = _rig(p)
    P, eng, ck = rig.P, rig.eng, rig.ck
    b = fhestr.narrow_default_bits(P, rig.pp, operand=True)
    msgs = (np.arange(64) * 7 + 3) % (P.msg_mod * P.carry_mod)
    d_cts = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_glwe = torch.zeros((fhestr.packed_glwe_len(P, 64),), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.pack(d_in=d_cts.data_ptr(), count=64, d_out=d_glwe.data_ptr())
    narrow = eng.narrow(d_glwe, 64, b)                      # narrowed where the packing wrote it
    assert eng.narrow_info()["kernel"] == "narrow" and narrow.nbytes == fhestr.narrow_len(P, 64, b) * 8
    eng.synchronize()
    _same(np.asarray(narrow).reshape(-1), fhestr.glwe_narrow_host(P, d_glwe.cpu().numpy().view(np.uint64), 64, b), "device against the host loop")
    assert np.array_equal(ck.decrypt_narrow(narrow), msgs)
    lwes = eng.unpack_narrow(narrow, refresh=False)
    assert eng.narrow_info() == {"ran": True, "kernel": "extract", "items": 64, "workgroups": 64, "bits": b}
    assert np.array_equal(ck.decrypt(lwes), msgs)
    _same(lwes, fhestr.narrow_sample_extract_host(P, narrow, 64, b, 64), "device against the host loop")
    _same(eng.unpack_narrow(narrow, count=10, first=54, refresh=False), lwes[54:], "first = 54")


def test_refresh():
    import fhestr
    rig = _rig(P22)
    P, eng, ck = rig.P, rig.eng, rig.ck
    b = fhestr.narrow_default_bits(P, rig.pp, operand=True)
    assert (rig.pp, b) == ((7, 3), 16)
    M, B = P.msg_mod * P.carry_mod, 70
    msgs = (np.arange(B) * 3 + 2) % M
    narrow = eng.narrow(eng.pack(ck.encrypt(msgs)), B, b)
    fresh = eng.unpack_narrow(narrow)                       # refresh=True is the default
    assert eng.narrow_info() == {"ran": True, "kernel": "extract", "items": B, "workgroups": B, "bits": b}
    assert np.array_equal(ck.decrypt(fresh), msgs)
    assert not np.array_equal(fresh, eng.unpack_narrow(narrow, refresh=False))
    f = lambda x: (5 * x + 3) % M
    lut_id, _ = eng.generate_lookup_table(f)
    again = eng.apply_lookup_table(fresh, np.full(B, lut_id, dtype=np.uint32))
    assert np.array_equal(ck.decrypt(again), np.array([f(int(m)) for m in msgs]))


def test_refresh_refusals():
    import fhestr
    # no packing key
    eng = _engine(256, 1)
    _, narrow, _ = _case(256, 1, 257, 16)
    with pytest.raises(fhestr.FheError, match="packing key"):
        eng.unpack_narrow(narrow, 257, 16, count=3, refresh=True)
    rig = _rig(P22)
    P, eng, ck = rig.P, rig.eng, rig.ck
    msgs = np.arange(8) % 16
    glwes = eng.pack(ck.encrypt(msgs))
    # one bit below the operand-grade default
    b = fhestr.narrow_default_bits(P, rig.pp, operand=True)
    below = eng.narrow(glwes, 8, b - 1)
    before = eng.narrow_info()
    with pytest.raises(fhestr.FheError, match=r"refresh refused.*15 bits.*\(7, 3\)"):
        eng.unpack_narrow(below)
    assert eng.narrow_info() == before                      # refused before anything was launched
    assert np.array_equal(ck.decrypt(eng.unpack_narrow(below, refresh=False)), msgs)
    # the pair (7, 2): no width is operand-grade (the key's words do not matter to the judgement)
    try:
        eng.load_packing_key((7, 2), np.zeros(fhestr.packing_key_len(P, (7, 2)), dtype=np.uint64))
        with pytest.raises(fhestr.FheError, match=r"refresh refused.*\(7, 2\)"):
            eng.unpack_narrow(eng.narrow(glwes, 8, 32))
        with pytest.raises(fhestr.FheError, match=r"\(7, 2\)"):
            eng.narrow(glwes, 8)                            # bits=None asks for the operand-grade default
    finally:
        rig.load()


def test_raw_noise():
    """2,048 PBS outputs of PARAM_MESSAGE_2_CARRY_2 of known messages, packed on the device under (7, 3), narrowed at the
    operand-grade default (16 bits) and extracted raw.  Model: narrow_noise's out[0] * V_pbs, of which the narrowing's
    (1 + kN/2) / 12 * 2^-32 is 35.3 of 36.3 nominal variances: this checks V_narrow on real keys.  Band: +-15 %, the one
    tests/test_gpu_glwe_extract.py::test_raw_noise uses for the same sample count.
    Every output is packed into a GLWE of its own (2,048 launches of one block each).  The model's figure is a block's
    variance over masks; the blocks of ONE narrowed GLWE share its mask's rounding errors -- block c sees
    sum_i s_i e_(c-i), and the half of it that the key's mean carries is a random walk in c -- so the spread across the
    coefficients of a single GLWE is not that variance: its expectation is (1/4 + 1/6) / (1/2) = 0.83 of it with a wide
    scatter.  Measured so on the MI355X, all 2,048 in one GLWE: variance 1.313e-08 against the model's 2.047e-08, ratio 0.64.
    The same 2,048 blocks under masks of their own are independent samples, which the band assumes."""
    import fhestr
    import torch
    rig = _rig(P22)
    P, eng = rig.P, rig.eng
    b = fhestr.narrow_default_bits(P, rig.pp, operand=True)
    M, B, big = P.msg_mod * P.carry_mod, P.N, P.big_size
    msgs = (np.arange(B) * 5 + 1) % M
    lut_id, _ = eng.generate_lookup_table(lambda x: x)
    d_in = torch.from_numpy(rig.ck.encrypt(msgs).view(np.int64)).cuda()
    d_idx = torch.full((B,), lut_id, dtype=torch.int32).cuda()
    d_mid = torch.zeros_like(d_in)
    glwe_len, list_len = fhestr.packed_glwe_len(P, 1), fhestr.narrow_len(P, 1, b)
    d_glwe = torch.zeros((B, glwe_len), dtype=torch.int64).cuda()
    d_narrow = torch.zeros((B, list_len), dtype=torch.int64).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_mid.data_ptr(), B)
    for j in range(B):
        eng.pack(d_in=d_mid.data_ptr() + 8 * big * j, count=1, d_out=d_glwe.data_ptr() + 8 * glwe_len * j)
        eng.narrow(d_in=d_glwe.data_ptr() + 8 * glwe_len * j, held=1, bits=b, d_out=d_narrow.data_ptr() + 8 * list_len * j)
        eng.unpack_narrow(d_in=d_narrow.data_ptr() + 8 * list_len * j, held=1, bits=b, refresh=False, d_out=d_out.data_ptr() + 8 * big * j)
    eng.synchronize()
    assert eng.narrow_info() == {"ran": True, "kernel": "extract", "items": 1, "workgroups": 1, "bits": b}
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(rig.ck.decrypt(raw), msgs)
    err = rig.phase_errors(raw, msgs)
    nominal = fhestr.narrow_noise(P, rig.pp, b)[0]
    model = nominal * fhestr.noise_model(P)["v_pbs"]
    # the same blocks in ONE GLWE, for the record only (see above)
    eng.pack(d_in=d_mid.data_ptr(), count=B, d_out=d_glwe.data_ptr())
    one = eng.unpack_narrow(eng.narrow(d_glwe[:1], B, b), refresh=False)
    shared = rig.phase_errors(one, msgs)
    print(f"raw narrow unpack noise {P.name} pp={rig.pp} b={b}: variance {err.var():.4e} (mean {err.mean():.2e}), model {model:.4e} = "
          f"{nominal:.1f} nominal, ratio {err.var() / model:.4f}; key weight {int(rig.glwe_sk.sum())} of {P.k * P.N}; "
          f"all {B} in one GLWE (one mask): variance {shared.var():.4e}, ratio {shared.var() / model:.4f}")
    assert abs(err.var() / model - 1) <= 0.15


def test_string_operations_p22():
    import fhestr
    rig = _rig(P22)
    P, eng, ck = rig.P, rig.eng, rig.ck
    ops = fhestr.FheStringOps(eng)
    b = fhestr.narrow_default_bits(P, rig.pp, operand=True)
    enc = lambda t, c: ck.encrypt(fhestr.string_to_blocks(P, t, c))
    text = b"a quick brown fox"
    cap = 32
    n_blocks = cap * ops.bpc
    assert n_blocks == 128
    hay = enc(text, cap)
    up = ops.to_upper(hay, packed=fhestr.Narrow())
    assert eng.narrow_info()["kernel"] == "narrow" and eng.narrow_info()["bits"] == b
    assert isinstance(up, fhestr.NarrowString) and (up.count, up.capacity, up.bits) == (n_blocks, cap, b)
    assert up.nbytes == fhestr.narrow_len(P, 128, b) * 8                         # what crosses PCIe and what a service stores
    got = ops.contains(up, b"BROWN")                         # the narrow result straight back in
    assert eng.narrow_info() == {"ran": True, "kernel": "extract", "items": n_blocks, "workgroups": n_blocks, "bits": b}
    assert ck.decrypt(got.reshape(1, -1))[0] == 1
    assert ck.decrypt(ops.contains(up, enc(b"brown", 8)).reshape(1, -1))[0] == 0
    client = ops.to_upper(hay, packed=fhestr.Narrow(13))
    assert client.bits == 13 and client.nbytes == fhestr.narrow_len(P, 128, 13) * 8
    assert fhestr.blocks_to_string(P, ck.decrypt_narrow(client)) == text.upper()
    # the split family: count and parts are NarrowStrings and go back in as operands
    res = ops.split(hay, b" ", 4, packed=fhestr.Narrow())
    assert isinstance(res.count, fhestr.NarrowString) and all(isinstance(x, fhestr.NarrowString) and x.capacity == cap for x in res.parts)
    assert fhestr.decode_count(P, ck.decrypt_narrow(res.count)) == 4
    assert [fhestr.blocks_to_string(P, ck.decrypt_narrow(x)) for x in res.parts] == text.split(b" ")
    assert [int(ck.decrypt(ops.contains(x, b"brown").reshape(1, -1))[0]) for x in res.parts[1:3]] == [0, 1]
    # op_many over NarrowString rows
    many = ops.op_many("contains", [up, res.parts[2]], b"BROWN")
    assert many.shape == (2, 1, P.big_size) and ck.decrypt(many[:, 0]).tolist() == [1, 0]
    with pytest.raises(fhestr.FheError, match="refresh refused"):
        ops.contains(client, b"BROWN")                       # client-grade width: not an operand
    lower = ops.op_many("to_lower", [up, res.parts[3]], packed=fhestr.Narrow())
    dec = ck.decrypt_narrow(lower)
    assert [fhestr.blocks_to_string(P, dec[:n_blocks]), fhestr.blocks_to_string(P, dec[n_blocks:])] == [text, b"fox"]
    ops.close()
