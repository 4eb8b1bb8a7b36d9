"""The packing keyswitch on the GPU (csrc/packing_ks_kernels.hip.h, Packing::pack_dev) against exact integers
(tests/exact_packing.py).  Every comparison is equality of all words of all GLWEs; every check prints and asserts
fhe_engine_packing_info (row tiles per workgroup, K chunks, K steps per chunk).  Shapes are the smallest at which the
kernel can still go wrong:

  test_rotation_and_wrap    toy twin N = 256, k = 5 (the body polynomial at column offset 5 N), count = N: every degree
                            0 .. N - 1 occurs, every tile has wrapped and unwrapped anti-diagonals; edge rows first
  test_ragged_counts        count = 1, 31, 33, N - 1
  test_several_glwes        count = N + 1 and 2 N + 37: the last GLWE's unused coefficients are exactly 0
  test_other_shapes         k = 1, N = 2048 and k = 2, N = 1024 toy-n twins, count = 257: MT 8, grid.y = 2, a ragged tile
  test_levels_and_chunks    (7, 2), (3, 5), (1, 16) x FHESTR_KS_CHUNKS = 1, the clamped maximum, a last chunk shorter than DEPTH
  test_edge_material        edge key x edge rows: accumulator columns at their extreme magnitude and sign
  test_buffer_reuse         2 N + 37, 5, 2 N + 37 LWEs on one engine
  test_key_replaced_digits_grown  (7, 2) then (3, 5) on one engine: the first key's digit buffer is dropped, the second's is
                            allocated for 5 LWEs, grown for 2 N + 37, reused for 5
  test_n8192_three_levels   the default (7, 3) of the N = 8192 sets: a 3.2 GB key, 3.4 GB of digit planes, sparse masks
  test_device_path          pack_lwes_dev on the buffer fhe_ks_pbs_batch_dev just wrote = the host loop on the downloaded
                            LWEs (fhe_packing_keyswitch_host) = the host-array entry point; also with throughput mode 1 on
  test_host_staging_grows_under_throughput_mode  the host-array entry point grows its staging while a pipelined call's
                            streams are live, then reuses it
  test_engine_close_...     the packed route's cached plans are destroyed before their engine
  test_end_to_end           toy-n twin of PARAM_MESSAGE_2_CARRY_2, device-generated server keys: to_lower and eq with
                            packed=True, decrypt_packed = Python bytes semantics = the unpacked run's decryption"""
import numpy as np
import pytest

import oracle as O
from exact_packing import ExactPacking, edge_pack_cts, edge_pksk, sparse_case

pytestmark = pytest.mark.gpu

P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS
P21 = O.PARAM_MESSAGE_2_CARRY_1_KS_PBS
K5 = next(p for p in O.TOY_SHAPES if p.name == "TOY_N256_K5")                  # k = 5, N = 256
N2048 = O.Params(8, P22.k, P22.N, P22.pbs_base_log, P22.pbs_level, P22.ks_base_log, P22.ks_level, 4, 4, P22.lwe_std, P22.glwe_std,
                 "TOY_N2048_K1")
N1024 = O.Params(8, P21.k, P21.N, P21.pbs_base_log, P21.pbs_level, P21.ks_base_log, P21.ks_level, 4, 2, P21.lwe_std, P21.glwe_std,
                 "TOY_N1024_K2_n8")
# the end-to-end twin: PARAM_MESSAGE_2_CARRY_2's GLWE side, n = 16 and the toy shapes' noise
E2E = O.Params(16, 1, 2048, 23, 1, 3, 5, 4, 4, 1e-13, 1e-17, "TOY_N2048_K1_n16")


def _fp(p):
    import fhestr
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name)


def _seed(p, pp, *more):
    return [p.N, p.k, pp[0], pp[1], *more]


class _Rig:
    """An engine under chosen environment switches with a packing key, and the exact reference under the same key."""

    def __init__(self, monkeypatch, p, pp, env, key):
        import fhestr
        self.p = p
        for name, value in env:
            monkeypatch.setenv(name, str(value))
        self.eng = fhestr.Engine(_fp(p), 0)
        assert not self.eng.packing_info()["ran"]
        self.load(pp, key)

    def load(self, pp, key="uniform"):
        """A key for the decomposition pp, replacing whatever the engine held; nothing has run under it yet."""
        p, self.pp = self.p, pp
        rng = np.random.default_rng(_seed(p, pp, 77))
        self.key = (edge_pksk(p, pp, rng) if key == "edge" else
                    rng.integers(0, 2**64, size=(p.k * p.N * pp[1], p.k + 1, p.N), dtype=np.uint64))
        self.eng.load_packing_key(pp, self.key)
        assert not self.eng.packing_info()["ran"]
        self.ref = ExactPacking(p, pp, self.key)

    def inputs(self, B, salt=0):
        return edge_pack_cts(self.p, self.pp, np.random.default_rng(_seed(self.p, self.pp, B, salt)), B)


_RIGS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for rig in _RIGS.values():
        rig.eng.close()
    _RIGS.clear()


def _rig(monkeypatch, p, pp, env=(), key="uniform"):
    k = (p.name, pp, tuple(env), key)
    if k not in _RIGS:
        _RIGS[k] = _Rig(monkeypatch, p, pp, env, key)
    return _RIGS[k]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _steps(p, pp):
    return -(-p.k * p.N // (2 * (16 // pp[1])))


def _geometry(p, pp, B, override=0):
    """The host arithmetic of Packing::pack_dev, from the parameters: (MT, chunks, steps per chunk, steps)."""
    steps = _steps(p, pp)
    col_groups = (p.k + 1) * p.N // 32
    row_tiles = -(-B // 32)
    mt = 1
    while mt < 8 and mt < row_tiles:
        mt *= 2
    gy = -(-row_tiles // mt)
    chunks = override or (6 * _cus() + col_groups * gy * mt // 2) // (col_groups * gy * mt)
    chunks = max(1, min(chunks, (steps + 7) // 8))
    chunks = max(chunks, -(-steps // ((1 << (20 - pp[0])) - 1)))
    spc = -(-steps // chunks)
    return mt, -(-steps // spc), spc, steps


def _assert_words(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad):
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ from exact; first (glwe, polynomial, coefficient) "
                             f"{bad[:12].tolist()}; polynomials {np.unique(bad[:, 1]).tolist()}, coefficients "
                             f"{np.unique(bad[:, 2])[:16].tolist()}")


def _check(rig, B, test, override=0, salt=0):
    cts = rig.inputs(B, salt)
    got = rig.eng.pack(cts)
    info = rig.eng.packing_info()
    print(f"pack-path {test} {rig.p.name} pp={rig.pp} B={B}: tile={info['tile']} chunks={info['chunks']} "
          f"steps_per_chunk={info['steps_per_chunk']} last_chunk={info['last_chunk']} of {info['steps']}")
    mt, chunks, spc, steps = _geometry(rig.p, rig.pp, B, override)
    assert (info["ran"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == (True, mt, chunks, spc, steps)
    assert mt == min(8, 1 << max(0, (-(-B // 32) - 1).bit_length()))
    want = rig.ref(cts)
    _assert_words(got, want, f"{rig.p.name} pp={rig.pp} B={B} {info}")
    return info, got


def test_rotation_and_wrap(monkeypatch):
    rig = _rig(monkeypatch, K5, (5, 2))
    info, got = _check(rig, K5.N, "rotation_and_wrap")
    assert info["tile"] == 8 and got.shape == (1, 6, 256)


@pytest.mark.parametrize("B", [1, 31, 33, K5.N - 1], ids=lambda b: f"B{b}")
def test_ragged_counts(monkeypatch, B):
    info, _ = _check(_rig(monkeypatch, K5, (5, 2)), B, "ragged_counts")
    assert info["tile"] == {1: 1, 31: 1, 33: 2, 255: 8}[B]


@pytest.mark.parametrize("B", [K5.N + 1, 2 * K5.N + 37], ids=lambda b: f"B{b}")
def test_several_glwes(monkeypatch, B):
    _, got = _check(_rig(monkeypatch, K5, (5, 2)), B, "several_glwes")
    assert got.shape[0] == -(-B // K5.N)
    # the keyswitch of nothing: with the mask rows of the last GLWE's LWEs removed nothing but their own terms remains, so
    # the exact reference (asserted equal above) holds the statement; a GLWE packed from zero LWEs is zero everywhere
    rig = _rig(monkeypatch, K5, (5, 2))
    zero = np.zeros((B, K5.k * K5.N + 1), dtype=np.uint64)
    zero[:, -1] = np.arange(1, B + 1, dtype=np.uint64)                          # zero masks: T_d = (0, ..., body_d)
    got = rig.eng.pack(zero)
    bodies = np.zeros(got.shape[0] * K5.N, dtype=np.uint64)
    bodies[:B] = np.arange(1, B + 1, dtype=np.uint64)
    want = np.zeros_like(got)
    want[:, K5.k, :] = bodies.reshape(-1, K5.N)
    _assert_words(got, want, f"zero masks B={B}")
    assert not got[-1, :, B % K5.N:].any(), "unused coefficients of the last GLWE are not 0"


@pytest.mark.parametrize("p,pp", [(N2048, (7, 2)), (N1024, (6, 3))], ids=["N2048_K1", "N1024_K2"])
def test_other_shapes(monkeypatch, p, pp):
    info, _ = _check(_rig(monkeypatch, p, pp), 257, "other_shapes")
    assert info["tile"] == 8                                                    # 9 row tiles: grid.y = 2, the second ragged


def _short_last_chunk(steps, depth):
    """An FHESTR_KS_CHUNKS value whose last chunk is shorter than the pipeline depth (and not empty), or None."""
    for c in range(2, (steps + 7) // 8 + 1):
        spc = -(-steps // c)
        last = steps - (-(-steps // spc) - 1) * spc
        if 0 < last < depth:
            return c
    return None


# B = 129: five row tiles, MT 8, DEPTH 4.  The shape per decomposition is the first of these on which some FHESTR_KS_CHUNKS
# leaves a last chunk of 1 .. 3 steps (80 steps of (7, 2) on the k = 5 twin admit none: 128 steps of the N = 2048 twin do).
def _chunk_shape(pp):
    for p in (K5, N2048, N1024):
        c = _short_last_chunk(_steps(p, pp), 4)
        if c:
            return p, c
    raise AssertionError(f"no shape with a short last chunk for {pp}")


@pytest.mark.parametrize("which", ["one", "clamped", "short_last"])
@pytest.mark.parametrize("pp", [(7, 2), (3, 5), (1, 16)], ids=str)
def test_levels_and_chunks(monkeypatch, pp, which):
    p, short = _chunk_shape(pp)
    steps = _steps(p, pp)
    override = {"one": 1, "clamped": 1000, "short_last": short}[which]
    info, _ = _check(_rig(monkeypatch, p, pp, env=(("FHESTR_KS_CHUNKS", override),)), 129, f"levels_and_chunks[{which}]", override=override)
    assert info["tile"] == 8 and info["steps"] == steps
    if which == "one":
        assert info["chunks"] == 1 and info["steps_per_chunk"] == steps
    elif which == "clamped":
        assert info["chunks"] <= (steps + 7) // 8 < 1000 and info["steps_per_chunk"] == 8
    else:
        assert 0 < info["last_chunk"] < 4, info
    if pp == (1, 16):
        assert steps == p.k * p.N // 2                                          # one mask element per 16-slot group


@pytest.mark.parametrize("env", [(), (("FHESTR_KS_CHUNKS", 1),)], ids=["auto", "one-chunk"])
@pytest.mark.parametrize("p,pp", [(K5, (7, 2)), (N2048, (7, 2)), (K5, (3, 5))], ids=["K5-7x2", "N2048-7x2", "K5-3x5"])
def test_edge_material(monkeypatch, p, pp, env):
    """Key columns whose eight balanced base-256 digits are all -128 (and the other EDGE_KEY_WORDS) at both ends of every
    polynomial, against rows of extreme digits: k N = 2048, base 7 x 2 levels in one chunk puts 2048 * (64 + 63) * 128 =
    2^24.99 into an int32 accumulator."""
    rig = _rig(monkeypatch, p, pp, env=env, key="edge")
    for B in (14, 45):
        _check(rig, B, "edge_material", override=1 if env else 0)


def test_buffer_reuse(monkeypatch):
    rig = _rig(monkeypatch, K5, (5, 2))
    for salt, B in enumerate((2 * K5.N + 37, 5, 2 * K5.N + 37)):
        _check(rig, B, "buffer_reuse", salt=salt + 1)


def test_key_replaced_digits_grown(monkeypatch):
    """The digit fragments' pad slots depend on the level count: a new key drops the buffer.  test_buffer_reuse starts at its
    largest batch; here the buffer of the second key starts small and has to grow."""
    rig = _Rig(monkeypatch, K5, (7, 2), (), "uniform")       # an engine of its own: the shared rigs keep their key
    try:
        _check(rig, 5, "key_replaced_digits_grown")
        rig.load((3, 5))
        for salt, B in enumerate((5, 2 * K5.N + 37, 5)):
            _check(rig, B, "key_replaced_digits_grown", salt=salt + 1)
    finally:
        rig.eng.close()


def test_n8192_three_levels():
    """PARAM_MULTI_BIT_MESSAGE_3_CARRY_3's default decomposition on the toy-n twin of its shape: 820 K steps of five mask
    elements (one pad slot per group, two ragged elements in the last), 512 column groups.  The whole key cannot be multiplied
    exactly in a test's time: masks are zero outside 48 positions, the key rows of those alone are drawn (sparse_case)."""
    import fhestr
    p, pp = O.TOY_N8192, (7, 3)
    assert fhestr.packing_default_params(fhestr.PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS) == pp
    key, cts, want = sparse_case(p, pp, 37)
    eng = fhestr.Engine(_fp(p), 0)
    try:
        eng.load_packing_key(pp, key)
        del key
        got = eng.pack(cts)
        info = eng.packing_info()
        print(f"pack-path n8192_three_levels {p.name} pp={pp} B=37: {info}")
        assert (info["ran"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == (True, *_geometry(p, pp, 37))
        assert info["steps"] == 820
        _assert_words(got, want, f"{p.name} pp={pp} B=37 {info}")
    finally:
        eng.close()


# ---- with real keys: the device path and whole string operations -----------------------------------------------------------------

class _E2E:
    def __init__(self):
        import fhestr
        self.P = _fp(E2E)
        self.ck = fhestr.ClientKey(self.P, 0x5EED0900)
        self.eng = fhestr.Engine(self.P, 0)
        glwe_sk, small_sk = self.ck.secret_keys()
        self.eng.generate_keys(glwe_sk, small_sk, 0x5EED0901)
        self.pp, self.key = self.ck.gen_packing_key(seed=0x5EED0902)
        self.eng.load_packing_key(self.pp, self.key)


_E2E_RIG = []


@pytest.fixture(scope="module")
def e2e():
    if not _E2E_RIG:
        _E2E_RIG.append(_E2E())
    yield _E2E_RIG[0]


@pytest.fixture(scope="module", autouse=True)
def _close_e2e():
    yield
    for r in _E2E_RIG:
        r.eng.close()
        r.ck.close()
    _E2E_RIG.clear()


def test_device_path(e2e):
    import torch
    P, eng, ck = e2e.P, e2e.eng, e2e.ck
    M = P.msg_mod * P.carry_mod
    B = 70
    msgs = (np.arange(B) * 5 + 1) % M
    lut_id, _ = eng.generate_lookup_table(lambda x: (3 * x + 1) % M)
    d_in = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_idx = torch.full((B,), lut_id, dtype=torch.int32).cuda()
    d_out = torch.zeros_like(d_in)
    d_glwe = torch.zeros((1, P.k + 1, P.N), dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), B)
    eng.pack(d_in=d_out.data_ptr(), count=B, d_out=d_glwe.data_ptr())          # enqueued behind the rotation, no synchronisation
    info = eng.packing_info()
    eng.synchronize()
    print(f"pack-path device_path {P.name} pp={e2e.pp} B={B}: {info}")
    assert (info["ran"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == (True, *_geometry(E2E, e2e.pp, B))
    lwes = d_out.cpu().numpy().view(np.uint64)
    got = d_glwe.cpu().numpy().view(np.uint64)
    import fhestr
    _assert_words(got, fhestr.packing_keyswitch_host(P, e2e.pp, e2e.key, lwes), "device path against the host loop on the downloaded LWEs")
    _assert_words(eng.pack(lwes), got, "host-array entry point against the device path")
    _assert_words(eng.pack(d_out, count=B), got, "tensor form against the pointer form")
    want = (3 * msgs + 1) % M
    assert np.array_equal(ck.decrypt(lwes), want)
    assert np.array_equal(ck.decrypt_packed(got, B), want)
    # throughput mode 1: the rotation that writes d_out may run beside another stream's keyswitch; pack waits for all of them
    d_glwe2 = torch.zeros_like(d_glwe)
    torch.cuda.synchronize()
    eng.set_pipeline(1)
    try:
        for _ in range(2):
            eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), B)
        eng.pack(d_in=d_out.data_ptr(), count=B, d_out=d_glwe2.data_ptr())
        eng.synchronize()
    finally:
        eng.set_pipeline(0)
    lwes2 = d_out.cpu().numpy().view(np.uint64)
    _assert_words(d_glwe2.cpu().numpy().view(np.uint64), fhestr.packing_keyswitch_host(P, e2e.pp, e2e.key, lwes2), "packing behind pipelined calls")


def test_host_staging_grows_under_throughput_mode(e2e):
    """fhe_engine_pack_lwes replaces its staging buffers while the streams of a pipelined call are live (it waits for them
    first), then reuses them for a smaller batch behind a second pipelined call."""
    import fhestr
    import torch
    P, eng, ck = e2e.P, e2e.eng, e2e.ck
    M = P.msg_mod * P.carry_mod
    B = 70
    msgs = (np.arange(B) * 5 + 1) % M
    lut_id, _ = eng.generate_lookup_table(lambda x: (3 * x + 1) % M)
    d_in = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_idx = torch.full((B,), lut_id, dtype=torch.int32).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    got = []
    eng.set_pipeline(1)
    try:
        for count in (150, 33):                             # 150: more than any host-array pack of this module before it
            host = ck.encrypt((np.arange(count) * 7 + 2) % M)
            eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), B)
            got.append((host, eng.pack(host)))
        eng.synchronize()
    finally:
        eng.set_pipeline(0)
    for host, glwes in got:
        info = f"{len(host)} host LWEs behind a pipelined call"
        _assert_words(glwes, fhestr.packing_keyswitch_host(P, e2e.pp, e2e.key, host), info)
    assert np.array_equal(ck.decrypt(d_out.cpu().numpy().view(np.uint64)), (3 * msgs + 1) % M)


def test_end_to_end(e2e):
    """Runs at k N = 2048: the CPU generation of the (7, 2) packing key takes about a second on 16 threads."""
    import fhestr
    P, eng, ck = e2e.P, e2e.eng, e2e.ck
    ops = fhestr.FheStringOps(eng)
    s, cap = b"Hi, ZoE!", 9
    enc = lambda t: ck.encrypt(fhestr.string_to_blocks(P, t, cap))
    es = enc(s)
    n_blocks = cap * fhestr.blocks_per_char(P)
    packed = ops.to_lower(es, packed=True)
    info = eng.packing_info()
    print(f"pack-path end_to_end to_lower {P.name} pp={e2e.pp} B={n_blocks}: {info}")
    assert (info["ran"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == (True, *_geometry(E2E, e2e.pp, n_blocks))
    assert packed.shape == (1, P.k + 1, P.N)
    plain = ops.to_lower(es)
    assert np.array_equal(ck.decrypt_packed(packed, n_blocks), ck.decrypt(plain))
    # the packed route runs the operation's plan on device buffers and packs its output there: the same plan, the same words
    _assert_words(packed, fhestr.packing_keyswitch_host(P, e2e.pp, e2e.key, plain), "packed to_lower against the host loop on the unpacked result")
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(packed, n_blocks)) == s.lower()
    for other in (s, b"Hi, ZoE?", b"Hi"):
        flag = ops.eq(es, enc(other), packed=True)
        info = eng.packing_info()
        assert (info["ran"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == (True, *_geometry(E2E, e2e.pp, 1))
        assert flag.shape == (P.k + 1, P.N)
        got = ck.decrypt_packed(flag, 1)[0]
        assert got == int(s == other) == ck.decrypt(ops.eq(es, enc(other)))[0]
    # many rows against one pattern, packed: output o of row r is block r * n_outputs + o
    rows = np.stack([enc(t) for t in (s, b"hi, zoe!", b"Hi")])
    flags = ops.op_many("eq", rows, enc(s), packed=True)
    assert flags.shape == (1, P.k + 1, P.N)
    assert ck.decrypt_packed(flags, 3).tolist() == [1, 0, 0] == ck.decrypt(ops.eq_many(rows, enc(s))).tolist()
    both = ops.strip_prefix(es, b"Hi", packed=True)
    dec = ck.decrypt_packed(both, 1 + n_blocks)
    assert dec[0] == 1 and fhestr.blocks_to_string(P, dec[1:]) == s[2:]


def test_engine_close_takes_the_cached_plans_first():
    """The packed route keeps its plans on the FheStringOps object; they point into the engine, so Engine.close destroys
    them before the engine, whatever order the objects are dropped in."""
    import fhestr
    P = _fp(O.TOY_K1)
    ck = fhestr.ClientKey(P, 0x5EED0A00)
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), 0x5EED0A01)
    eng.load_packing_key(*ck.gen_packing_key(seed=5))
    ops = fhestr.FheStringOps(eng)
    es = ck.encrypt(fhestr.string_to_blocks(P, b"Ab", 2))
    n = 2 * ops.bpc
    assert fhestr.blocks_to_string(P, ck.decrypt_packed(ops.to_upper(es, packed=True), n)) == b"AB"
    assert ops._plans
    eng.close()                                             # ops is still alive and held plans
    assert not ops._plans
    del ops
    ck.close()
