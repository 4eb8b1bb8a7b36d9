"""Every keyswitch path of Engine::launch_keyswitch (csrc/engine.hip) against exact integers (tests/exact_keyswitch.py).

Every comparison is equality of all words of all small ciphertexts; batches are all-distinct rows of edge_big_cts (the
first rows sit on the decomposer's edges, the rest are uniform).  Every test asserts through Engine.keyswitch_info()
(fhe_engine_keyswitch_info) which kernel ran, with how many row tiles per workgroup (MT), K chunks and steps per chunk,
and prints them ("ks-path ..." lines).  Environment switches are read in Engine::create: they are set around the
construction of a fresh engine; engines are kept for the module and closed at its end.

  matrix cores (ks_decompose_kernel + keyswitch_mfma_kernel<MT>; DEPTH 2 for MT <= 2, 4 above)
    test_mfma_real_dimensions   MT 1 / 2 / 4 / 8 by batch size, grid.y > 1 with a ragged last row tile (B = 257, 1027), ragged
                                last 16-slot group (PARAM_MESSAGE_2_CARRY_2, _2_CARRY_1), automatic K chunks
    test_mfma_chunk_overrides   FHESTR_KS_CHUNKS: one chunk, the clamped maximum, and values that leave every residue of the
                                last chunk's length modulo DEPTH, including a last chunk shorter than DEPTH (MT 2 and MT 8)
    test_clamped_chunks         ks_mfma_max_steps binds (k N = 32768, base 7 x 6 levels): two chunks where one was asked for
    test_mfma_large_n           k N = 8192, 16384, 32768 with 6 and 7 levels (two mask elements per group), two ragged column groups
    test_column_edges[mfma-*]   n + 1 = 32, 33, 256, 257: full and ragged last column group
    test_edge_material[mfma-*]  edge key x edge rows: accumulator columns at their extreme magnitude and sign
    test_buffer_reuse           1027, 5, 1027 LWEs on one engine: stale digit rows, no reallocation
  byte planes (keyswitch_dot4_kernel<8, 2>)
    test_dot4_real_dimensions   FHESTR_KS_MFMA=0: sample tiles of 8 (B = 1, 7, 8, 9, 37, 257)
    test_column_edges[dot4-*]   full and ragged 256-column tile
    test_dot4_many_levels       more than 16 levels (22 x base 1, 17 x base 2), 257 columns, no switch set
    test_edge_material[dot4-*]  u32 accumulators and the load-time bias correction at their extremes
  through apply_lookup_table_dev / _small_key (structured bootstrapping key: the output must be the exact PBS of the exact
  keyswitch, bit for bit -- tests/test_gpu_exact_rotation.py, tier 1.  The rotation reads only the top log2(2N) + 1 bits of
  every keyswitch word, so these see a wrong row, a dropped body or a wrong bias, not an error in the low bits: the low
  bits of the shadow kernel's code are those of test_dot4_*, of the matrix cores' those above)
    test_shadow_kernel          set_pipeline(1): keyswitch_dot4_kernel<4, 8> beside the previous call's rotation, B = 96 and 3
    test_overlapped_mode_growing_batches   set_pipeline(2): a digit buffer per stream, reallocated when a larger batch arrives
    test_overlapped_mode_three_and_four_streams   FHESTR_OVERLAP_STREAMS = 3, 4: nine calls of 5 / 96 / 37 LWEs over every lane
    test_overlapped_mode_every_lane_grows   the same engines: a round of 5 LWEs per lane, then a round of 130
    test_overlapped_mode_dependent_calls   the same two engines: a chain, two calls into one buffer, an overwritten input -- against
                                serial calls on the same kernel (variant selector 16 | 2), five times over
    test_small_key_right_after_shadow_calls   apply_lookup_table_small_key at once after four set_pipeline(1) calls: its second
                                small-ciphertext buffer is the one those calls use
    test_small_key_order        blind rotation first, then the keyswitch of its output buffer"""
import numpy as np
import pytest

import oracle as O
from exact_keyswitch import ExactKeyswitch, edge_big_cts, edge_ksk
from exact_pbs import edge_small_cts, pbs_exact_batch, pbs_exact_batch_parallel, structured_bsk

pytestmark = pytest.mark.gpu

N_LUTS = 3


def _twin(p, n, name, ks=None):
    bl, L = ks or (p.ks_base_log, p.ks_level)
    return O.Params(n, p.k, p.N, p.pbs_base_log, p.pbs_level, bl, L, p.msg_mod, p.carry_mod, p.lwe_std, p.glwe_std, name)


def _shape(name):
    return next(p for p in O.TOY_SHAPES if p.name == name)


P22 = O.PARAM_MESSAGE_2_CARRY_2_KS_PBS                             # base 3 x 5 levels: 3 elements per group, 2048 = 341 * 6 + 2
P21 = O.PARAM_MESSAGE_2_CARRY_1_KS_PBS                             # k = 2, base 4 x 3 levels: 5 per group, 2048 = 204 * 10 + 8
B7 = _twin(P22, 888, "N2048_n888_KS2x7", ks=(7, 2))                # PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3's keyswitch: the largest digits
LARGE = [_twin(O.TOY_N8192, 40, "N8192_n40_KS6x3"), _twin(_shape("TOY_N16384_L2"), 40, "N16384_n40_KS6x3"),
         _twin(O.TOY_N32768, 40, "N32768_n40_KS7x3")]
CLAMP = _twin(O.TOY_N32768, 40, "N32768_n40_KS6x7", ks=(7, 6))
COLS = [_twin(P22, c - 1, f"N2048_cols{c}") for c in (32, 33, 256, 257)]
MANY = [_twin(P22, 256, f"N2048_cols257_KS{L}x{bl}", ks=(bl, L)) for bl, L in ((1, 22), (2, 17))]
N2048 = _twin(P22, 8, "TOY_N2048_K1")
N1024 = _twin(P21, 8, "TOY_N1024_K2_n8")


def _fp(p):
    import fhestr
    return fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                         p.lwe_std, p.glwe_std, p.name)


def _seed(p, *more):
    return [p.N, p.k, p.n, p.ks_base_log, p.ks_level, *more]


class _Rig:
    """An engine under chosen environment switches with a keyswitch key, and the exact reference under the same key."""

    def __init__(self, monkeypatch, p, env, key, structured):
        import fhestr
        self.p = p
        self.rng = np.random.default_rng(_seed(p, len(key)))
        ksk_rng = np.random.default_rng(_seed(p, 77))
        self.ksk = (edge_ksk(p, ksk_rng) if key == "edge" else
                    ksk_rng.integers(0, 2**64, size=(p.k * p.N * p.ks_level, p.n + 1), dtype=np.uint64))
        if structured:
            bsk, self.terms, _ = structured_bsk(p, self.rng)
        else:                                                   # the rotation is not under test: any words
            bsk = self.rng.integers(0, 2**64, size=p.n * p.pbs_level * (p.k + 1) ** 2 * p.N, dtype=np.uint64)
        for name, value in env:
            monkeypatch.setenv(name, str(value))
        self.eng = fhestr.Engine(_fp(p), 0)
        self.eng.load_keys(bsk.reshape(-1), self.ksk.reshape(-1))
        self.ref = ExactKeyswitch(p, self.ksk)
        if structured:
            self.luts = self.rng.integers(0, 2**64, size=(N_LUTS, p.glwe_len), dtype=np.uint64)
            self.ids = np.array([self.eng.upload_lut(lut) for lut in self.luts], dtype=np.uint32)

    def inputs(self, B, salt=0):
        return edge_big_cts(self.p, np.random.default_rng(_seed(self.p, B, salt)), B)


_RIGS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for rig in _RIGS.values():
        rig.eng.close()
    _RIGS.clear()


def _rig(monkeypatch, p, env=(), key="uniform", structured=False):
    k = (p.name, tuple(env), key, structured)
    if k not in _RIGS:
        _RIGS[k] = _Rig(monkeypatch, p, env, key, structured)
    return _RIGS[k]


def _assert_words(got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        with np.errstate(over="ignore"):
            d = np.abs((got - want).astype(np.int64)).astype(np.float64)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ from exact in {len(np.unique(bad[:, 0]))} of {len(want)} "
                             f"LWEs; first (row, column) {bad[:12].tolist()}; rows {np.unique(bad[:, 0])[:16].tolist()}, columns "
                             f"{np.unique(bad[:, 1])[:16].tolist()}; max torus distance 2^{np.log2(d.max()):.1f}")


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _mfma_geometry(p, B, override=0):
    """The host arithmetic of Engine::launch_keyswitch, from the parameters: (MT, chunks, steps per chunk, steps)."""
    epg = 16 // p.ks_level
    steps = -(-p.k * p.N // (2 * epg))
    col_groups = -(-(p.n + 1) // 32)
    row_tiles = -(-B // 32)
    mt = 1
    while mt < 8 and mt < row_tiles:
        mt *= 2
    gy = -(-row_tiles // mt)
    chunks = override or (6 * _cus() + col_groups * gy * mt // 2) // (col_groups * gy * mt)
    chunks = max(1, min(chunks, (steps + 7) // 8))
    max_steps = (1 << (20 - p.ks_base_log)) - 1
    chunks = max(chunks, -(-steps // max_steps))
    spc = -(-steps // chunks)
    return mt, -(-steps // spc), spc, steps


def _report(test, p, B, info):
    print(f"ks-path {test} {p.name} B={B}: {info['kernel']} tile={info['tile']} chunks={info['chunks']} "
          f"steps_per_chunk={info['steps_per_chunk']} last_chunk={info['last_chunk']} of {info['steps']}")


def _check_mfma(rig, B, test, override=0, salt=0):
    cts = rig.inputs(B, salt)
    got = rig.eng.keyswitch(cts)
    info = rig.eng.keyswitch_info()
    _report(test, rig.p, B, info)
    mt, chunks, spc, steps = _mfma_geometry(rig.p, B, override)
    assert (info["kernel"], info["tile"], info["chunks"], info["steps_per_chunk"], info["steps"]) == ("mfma", mt, chunks, spc, steps)
    assert mt == min(8, 1 << max(0, (-(-B // 32) - 1).bit_length()))
    _assert_words(got, rig.ref(cts), f"{rig.p.name} B={B} {info}")
    return info


def _check_dot4(rig, B, test, salt=0):
    cts = rig.inputs(B, salt)
    got = rig.eng.keyswitch(cts)
    info = rig.eng.keyswitch_info()
    _report(test, rig.p, B, info)
    in_dim = rig.p.k * rig.p.N
    assert (info["kernel"], info["tile"], info["chunks"], info["steps_per_chunk"]) == ("dot4", 8, -(-in_dim // 64), 64)
    _assert_words(got, rig.ref(cts), f"{rig.p.name} B={B} {info}")


# ---- matrix cores -----------------------------------------------------------------------------------------------------------

REAL = [(P22, B) for B in (1, 31, 32, 33, 64, 65, 128, 129, 256, 257, 1027)] + [(P21, B) for B in (3, 65, 257)] + \
       [(B7, B) for B in (5, 33, 129, 1027)]


@pytest.mark.parametrize("p,B", REAL, ids=[f"{p.name}-B{B}" for p, B in REAL])
def test_mfma_real_dimensions(monkeypatch, p, B):
    info = _check_mfma(_rig(monkeypatch, p), B, "mfma_real_dimensions")
    assert info["tile"] == {1: 1, 3: 1, 5: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 4, 128: 4, 129: 8, 256: 8, 257: 8, 1027: 8}[B]


# PARAM_MESSAGE_2_CARRY_2 has 342 K steps.  Override -> (chunks, steps per chunk, last chunk): 1 -> (1, 342, 342), 2 -> (2, 171, 171),
# 4 -> (4, 86, 84), 21 -> (21, 17, 2), 32 -> (32, 11, 1), 1000 -> clamped to 43 = ceil(342 / 8) -> (43, 8, 6).  Last chunk modulo
# DEPTH = 2 (B = 33, MT 2): 0, 1, 0, 0, 1, 0, with 1 < DEPTH; modulo DEPTH = 4 (B = 129, MT 8): 2, 3, 0, 2, 1, 2, with 2 and 1 < DEPTH.
OVERRIDES = {1: (1, 342), 2: (2, 171), 4: (4, 84), 21: (21, 2), 32: (32, 1), 1000: (43, 6)}


@pytest.mark.parametrize("B,depth", [(33, 2), (129, 4)], ids=["B33-MT2-DEPTH2", "B129-MT8-DEPTH4"])
@pytest.mark.parametrize("override", sorted(OVERRIDES), ids=lambda c: f"chunks{c}")
def test_mfma_chunk_overrides(monkeypatch, override, B, depth):
    info = _check_mfma(_rig(monkeypatch, P22, env=(("FHESTR_KS_CHUNKS", override),)), B, "mfma_chunk_overrides", override=override)
    assert (info["chunks"], info["last_chunk"]) == OVERRIDES[override]
    assert info["tile"] == {33: 2, 129: 8}[B]
    print(f"ks-path   last chunk {info['last_chunk']} = {info['last_chunk'] % depth} mod DEPTH {depth}")


def test_chunk_overrides_cover_every_residue():
    last = [v[1] for v in OVERRIDES.values()]
    assert {x % 2 for x in last} == {0, 1} and {x % 4 for x in last} == {0, 1, 2, 3} and min(last) < 2 and sorted(last)[1] < 4


def test_clamped_chunks(monkeypatch):
    """8192 K steps of base 7: one more than ks_mfma_max_steps allows a workgroup, so FHESTR_KS_CHUNKS=1 runs two chunks.
    Edge key and edge rows: 2^29.6 in the int32 accumulators, the closest an accepted shape comes to 2^31."""
    rig = _rig(monkeypatch, CLAMP, env=(("FHESTR_KS_CHUNKS", 1),), key="edge")
    info = _check_mfma(rig, 3, "clamped_chunks", override=1)
    assert (info["chunks"], info["steps_per_chunk"], info["steps"]) == (2, 4096, 8192)


@pytest.mark.parametrize("p", LARGE, ids=lambda p: p.name)
@pytest.mark.parametrize("B", [3, 70], ids=lambda b: f"B{b}")
def test_mfma_large_n(monkeypatch, p, B):
    _check_mfma(_rig(monkeypatch, p), B, "mfma_large_n")


@pytest.mark.parametrize("p", COLS, ids=lambda p: p.name)
@pytest.mark.parametrize("kernel", ["mfma", "dot4"])
def test_column_edges(monkeypatch, kernel, p):
    if kernel == "mfma":
        _check_mfma(_rig(monkeypatch, p), 37, "column_edges")
    else:
        _check_dot4(_rig(monkeypatch, p, env=(("FHESTR_KS_MFMA", 0),)), 37, "column_edges")


@pytest.mark.parametrize("p", [P22, B7], ids=lambda p: p.name)
@pytest.mark.parametrize("kernel,env", [("mfma", ()), ("mfma", (("FHESTR_KS_CHUNKS", 1),)), ("dot4", (("FHESTR_KS_MFMA", 0),))],
                         ids=["mfma", "mfma-one-chunk", "dot4"])
def test_edge_material(monkeypatch, kernel, env, p):
    rig = _rig(monkeypatch, p, env=env, key="edge")
    for B in (14, 45):
        if kernel == "mfma":
            _check_mfma(rig, B, "edge_material", override=1 if env else 0)
        else:
            _check_dot4(rig, B, "edge_material")


def test_buffer_reuse(monkeypatch):
    rig = _rig(monkeypatch, P22)
    for salt, B in enumerate((1027, 5, 1027)):
        _check_mfma(rig, B, "buffer_reuse", salt=salt + 1)


# ---- byte planes --------------------------------------------------------------------------------------------------------------

DOT4 = [(p, B) for p in (P22, P21) for B in (1, 7, 8, 9, 37, 257)]


@pytest.mark.parametrize("p,B", DOT4, ids=[f"{p.name}-B{B}" for p, B in DOT4])
def test_dot4_real_dimensions(monkeypatch, p, B):
    _check_dot4(_rig(monkeypatch, p, env=(("FHESTR_KS_MFMA", 0),)), B, "dot4_real_dimensions")


@pytest.mark.parametrize("p", MANY, ids=lambda p: p.name)
def test_dot4_many_levels(monkeypatch, p):
    rig = _rig(monkeypatch, p)
    for B in (9, 37):
        _check_dot4(rig, B, "dot4_many_levels")


# ---- through the blind rotation: shadow kernel, overlapped mode, small-key order -----------------------------------------------

_EXACT = {}     # (shape, batches) -> the exact case below: rigs of one shape differ in their environment switches only


def _exact_case(rig, batches):
    """Distinct inputs per call, their table choices, exact keyswitch and exact PBS of it; computed once per shape and batch list."""
    p = rig.p
    k = (p.name, tuple(batches))
    if k not in _EXACT:
        big = [rig.inputs(B, salt=100 + i) for i, B in enumerate(batches)]
        sel = [(np.arange(B) + i) % N_LUTS for i, B in enumerate(batches)]
        smalls = [rig.ref(b) for b in big]
        want_all = pbs_exact_batch_parallel(p, rig.terms, np.concatenate(smalls), rig.luts, np.concatenate(sel))
        _EXACT[k] = (rig.ksk, rig.luts, big, sel, smalls, np.split(want_all, np.cumsum(batches)[:-1]))
    ksk, luts, big, sel, smalls, wants = _EXACT[k]
    assert np.array_equal(ksk, rig.ksk) and np.array_equal(luts, rig.luts), "the shared exact case is another key's"
    return big, sel, smalls, wants


def _pipelined_calls(eng):
    """Pipelined calls of the engine's current run (fhe_debug_pipeline_calls, c_api.cpp): a call that falls back to the serial
    path, and any synchronisation, ends the run and sets it to 0."""
    import fhestr
    return fhestr.lib().fhe_debug_pipeline_calls(eng._h)


def _through_rotation(rig, mode, batches, test, expect, all_pipelined=False):
    """Consecutive apply_lookup_table_dev calls under set_pipeline(mode), distinct inputs per call; every output against
    the exact PBS of the exact keyswitch.  expect(info, B) judges what the query reports after each call is enqueued.
    all_pipelined: every call must have taken the throughput mode, none the serial path."""
    import torch
    p = rig.p
    big, sel, smalls, wants = _exact_case(rig, batches)
    ins = [torch.from_numpy(b.view(np.int64)).cuda() for b in big]
    idx = [torch.from_numpy(rig.ids[s].astype(np.int32)).cuda() for s in sel]
    outs = [torch.zeros_like(t) for t in ins]
    torch.cuda.synchronize()                   # torch's stream is not ordered with the engine's
    infos = []
    rig.eng.set_pipeline(mode)
    try:
        for i, o, x, B in zip(ins, outs, idx, batches):
            rig.eng.apply_lookup_table_dev(i.data_ptr(), x.data_ptr(), o.data_ptr(), B)
            infos.append(rig.eng.keyswitch_info())
        taken = _pipelined_calls(rig.eng)
        rig.eng.synchronize()
    finally:
        rig.eng.set_pipeline(0)
    for info, B in zip(infos, batches):
        _report(test, p, B, info)
    for call, (info, B) in enumerate(zip(infos, batches)):
        expect(info, B, call)
    if all_pipelined:
        assert taken == len(batches), f"{taken} of {len(batches)} calls ran in throughput mode {mode} after the last serial one"
    for call, (o, want, small) in enumerate(zip(outs, wants, smalls)):
        got = o.cpu().numpy().view(np.uint64)
        # a wrong keyswitch word moves the rotation: name the LWEs, then the words
        _assert_words(got, want, f"{p.name} mode {mode} call {call} (B = {len(want)}, {infos[call]})")


@pytest.mark.parametrize("B", [96, 3], ids=lambda b: f"B{b}")
@pytest.mark.parametrize("p", [N2048, N1024, P22], ids=lambda p: p.name)
def test_shadow_kernel(monkeypatch, p, B):
    """Three calls: the second and third keyswitch run beside the rotation of the call before.  If the shadow kernel did not
    run the call fell back to the serial path (Engine::shadow_keyswitch_fits): that fails here, with the register count."""
    rig = _rig(monkeypatch, p, structured=True)

    def expect(info, B, call):
        assert info["kernel"] == "dot4_shadow" and info["tile"] == 4, (
            f"call {call}: the shadow keyswitch kernel did not run ({info}): the blind-rotation kernel's code object reports "
            f"{info['rotation_regs']} vector registers per lane; a 64-register wave must fit beside its waves in 512 per SIMD")
        assert info["chunks"] == p.k * p.N // 64
    _through_rotation(rig, 1, [B, B, B], "shadow_kernel", expect)


def test_overlapped_mode_growing_batches(monkeypatch):
    """set_pipeline(2), two streams: calls 0, 2, 4 use the engine's digit buffer, calls 1, 3 the second stream's own, which
    grows from 40 to 200 LWEs (reallocated while the other stream is busy); call 4 is smaller than what its buffer held."""
    rig = _rig(monkeypatch, N2048, structured=True)

    def expect(info, B, call):
        mt, chunks, spc, steps = _mfma_geometry(rig.p, B)
        assert (info["kernel"], info["tile"], info["chunks"], info["steps_per_chunk"]) == ("mfma", mt, chunks, spc)
    _through_rotation(rig, 2, [33, 40, 96, 200, 64], "overlapped_mode", expect)


STREAMS = [3, 4]


def _streams_rig(monkeypatch, ns):
    return _rig(monkeypatch, N2048, env=(("FHESTR_OVERLAP_STREAMS", ns),), structured=True)


def _expect_mfma(rig):
    def expect(info, B, call):
        mt, chunks, spc, steps = _mfma_geometry(rig.p, B)
        assert (info["kernel"], info["tile"], info["chunks"], info["steps_per_chunk"]) == ("mfma", mt, chunks, spc)
    return expect


@pytest.mark.parametrize("ns", STREAMS, ids=lambda n: f"streams{n}")
def test_overlapped_mode_three_and_four_streams(monkeypatch, ns):
    """set_pipeline(2) over three and four lanes (lanes 2 and 3 exist under these settings only).  Nine calls of 5, 96, 37 LWEs
    in turn.  With three lanes every lane keeps its batch size (lane 0: 5, lane 1: 96, lane 2: 37).  With four, lane 0 meets
    5, 96, 37 and lane 3 meets 5, 96: their small-ciphertext and digit buffers are replaced while the other lanes are busy;
    lane 1 (96, 37) and lane 2 (37, 5) do not grow -- test_overlapped_mode_every_lane_grows is for that."""
    rig = _streams_rig(monkeypatch, ns)
    _through_rotation(rig, 2, [5, 96, 37] * 3, f"overlapped_mode_{ns}_streams", _expect_mfma(rig), all_pipelined=True)


@pytest.mark.parametrize("ns", STREAMS, ids=lambda n: f"streams{n}")
def test_overlapped_mode_every_lane_grows(monkeypatch, ns):
    """One round of 5 LWEs on every lane, then one of 130 (more than any other call on these engines, five row tiles instead
    of one): in the second round every lane, lanes 2 and 3 included, replaces its small-ciphertext and its digit buffer while
    the calls of the other lanes are in flight."""
    rig = _streams_rig(monkeypatch, ns)
    _through_rotation(rig, 2, [5] * ns + [130] * ns, f"overlapped_mode_{ns}_streams_grow", _expect_mfma(rig), all_pipelined=True)


@pytest.mark.parametrize("ns", STREAMS, ids=lambda n: f"streams{n}")
def test_overlapped_mode_dependent_calls(monkeypatch, ns):
    """Eight dependent calls on the engines above: a chain of four (every call reads the previous call's output, on another
    lane), two calls into one output buffer, and a call that overwrites the input of the call before it.  Five times over
    in mode 2, bit for bit what the same calls give one after the other on the same kernel (variant selector 16 | 2, for
    the reference only: under a forced selector no call is eligible for mode 2).  Every mode-2 call must have been pipelined."""
    import torch
    rig = _streams_rig(monkeypatch, ns)
    eng, B = rig.eng, 37
    x = [torch.from_numpy(rig.inputs(B, salt=200 + i).view(np.int64)).cuda() for i in range(2)]
    idx = torch.from_numpy(rig.ids[np.arange(B) % N_LUTS].astype(np.int32)).cuda()
    names = [f"chain[{i}]" for i in range(4)] + ["same", "war_out", "scratch"]

    def run(mode):
        eng.set_pipeline(mode)
        try:
            chain = [torch.zeros_like(x[0]) for _ in range(4)]
            same, war_out, scratch = torch.zeros_like(x[0]), torch.zeros_like(x[0]), x[1].clone()
            torch.cuda.synchronize()            # torch's stream is not ordered with the engine's: its fills and the clone land first
            calls = [(x[0], chain[0]), (chain[0], chain[1]), (chain[1], chain[2]), (chain[2], chain[3]),
                     (x[0], same), (chain[0], same), (scratch, war_out), (x[0], scratch)]
            for src, dst in calls:
                eng.apply_lookup_table_dev(src.data_ptr(), idx.data_ptr(), dst.data_ptr(), B)
            taken = _pipelined_calls(eng)
            eng.synchronize()
        finally:
            eng.set_pipeline(0)
        return [t.cpu().numpy() for t in chain + [same, war_out, scratch]], taken

    eng.set_variant(16 | 2)                     # the serial reference on the kernel mode 2 uses
    try:
        want, taken = run(0)
    finally:
        eng.set_variant(0)
    assert taken == 0
    for rep in range(5):
        got, taken = run(2)
        assert taken == 8, f"{ns} streams, repetition {rep}: {taken} of 8 calls ran overlapped after the last serial one"
        differ = [(nm, int((a != b).any(axis=1).sum())) for nm, a, b in zip(names, want, got) if not np.array_equal(a, b)]
        assert not differ, f"{ns} streams, repetition {rep}: (output, LWEs that differ) {differ}"
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[4], want[0])     # the calls did compute something


def test_small_key_right_after_shadow_calls(monkeypatch):
    """apply_lookup_table_small_key writes its keyswitch into lane 1's small-ciphertext buffer, which every second
    set_pipeline(1) call uses as well.  Four such calls, then the small-key call at once -- no synchronisation by the test,
    the mode left on: the same words as before those calls.  (The call itself waits for the keyswitch stream before it
    enqueues anything, and mode 1's rotations are on the engine's stream: this pins which buffer is used and that the
    call ends the run, it cannot show a race.)"""
    import torch
    rig = _rig(monkeypatch, N2048, structured=True)
    p, eng, B = rig.p, rig.eng, 96
    small = edge_small_cts(p, np.random.default_rng(_seed(p, 70, 6)), 70)
    sel = rig.ids[np.arange(70) % N_LUTS]
    want = eng.apply_lookup_table_small_key(small, sel)
    ins = [torch.from_numpy(rig.inputs(B, salt=300 + i).view(np.int64)).cuda() for i in range(4)]
    outs = [torch.zeros_like(t) for t in ins]
    idx = torch.from_numpy(rig.ids[np.arange(B) % N_LUTS].astype(np.int32)).cuda()
    torch.cuda.synchronize()
    eng.set_pipeline(1)
    try:
        for i, o in zip(ins, outs):
            eng.apply_lookup_table_dev(i.data_ptr(), idx.data_ptr(), o.data_ptr(), B)
        info, taken = eng.keyswitch_info(), _pipelined_calls(eng)
        got = eng.apply_lookup_table_small_key(small, sel)
        assert _pipelined_calls(eng) == 0
    finally:
        eng.set_pipeline(0)
    assert info["kernel"] == "dot4_shadow" and taken == 4, f"the four calls did not all take mode 1: {taken}, {info}"
    _assert_words(got, want, f"{p.name} small-key order after four mode-1 calls")
    assert all(o.any().item() for o in outs)


def test_small_key_order(monkeypatch):
    """apply_lookup_table_small_key: the keyswitch reads the rotation's output buffer.  Exact keyswitch of the exact PBS."""
    rig = _rig(monkeypatch, N2048, structured=True)
    p = rig.p
    for B in (5, 70):
        small = edge_small_cts(p, np.random.default_rng(_seed(p, B, 5)), B)
        sel = np.arange(B) % N_LUTS
        got = rig.eng.apply_lookup_table_small_key(small, rig.ids[sel])
        info = rig.eng.keyswitch_info()
        _report("small_key_order", p, B, info)
        mt, chunks, spc, steps = _mfma_geometry(p, B)
        assert (info["kernel"], info["tile"], info["chunks"], info["steps_per_chunk"]) == ("mfma", mt, chunks, spc)
        _assert_words(got, rig.ref(pbs_exact_batch(p, rig.terms, small, rig.luts, sel)), f"{p.name} small-key order B={B}")
