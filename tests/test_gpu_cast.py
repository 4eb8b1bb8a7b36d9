"""Casting keys on the GPU (csrc/cast_dev.hip, csrc/cast_kernels.hip.h): the matrix-core product at the cast geometry and the
fused digit kernel word for word against tests/exact_cast.py, the follow-up tables and whole strings on toy twins, one
real-size cast per target, the refusals and the noise of a keyswitched block.  The host side is tests/test_cast_host.py."""
import dataclasses

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from exact_cast import TO_BIG, TO_SMALL, cast_exact, cast_packed_exact, digit_fragments, edge_cts, edge_key
from exact_extract import SHAPES, random_glwes

pytestmark = pytest.mark.gpu


def _f():
    import fhestr
    return fhestr


def _shape(k, N, name, msg=2, carry=2):
    """A source that is only dimensions: the product and the digit kernels read k and N of it, nothing else."""
    return O.Params(5, k, N, 10, 1, 4, 2, msg, carry, 1e-12, 1e-15, name)


ODD = _shape(1, 101, "ODD_N101")                         # k N = 101: no multiple of any 2 epg
K2 = _shape(2, 128, "SRC_K2_N128")                       # k N = 256: no multiple of 2 epg for 3 and 5 levels
N41 = dataclasses.replace(O.TOY_K1, n=40, name="TOY_K1_n40")                                             # TO_SMALL: 41 columns
N2049 = dataclasses.replace(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, n=12, name="TOY_N2048_n12")               # TO_BIG: 2049 columns, the last group one column

_ENGINES = {}


def _engine(p):
    """An engine of the destination's shape; no keys (the keyswitched rows need none)."""
    if p.name not in _ENGINES:
        _ENGINES[p.name] = _f().Engine(to_fhestr_params(p), 0)
    return _ENGINES[p.name]


def _cast_key(src, dst, pair, target, key):
    f = _f()
    cp = f.cast_default_params(to_fhestr_params(src), to_fhestr_params(dst), target, pair)
    return f.CastKey(_engine(dst), cp, key)


# ---- the product at the cast geometry ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst,pair,target,count", [
    (ODD, O.TOY_N8192, (7, 1), TO_SMALL, 1),        # 1 level (epg 16), 9 columns, one row
    (K2, N41, (4, 3), TO_SMALL, 33),                # 3 levels (epg 5, one empty slot), 41 columns, two row tiles
    (K2, N2049, (3, 5), TO_BIG, 37),                # 5 levels (epg 3, one empty slot), 2049 columns
    (ODD, N41, (1, 15), TO_SMALL, 37),              # 15 levels (epg 1, one empty slot)
    (ODD, O.TOY_N8192, (1, 16), TO_SMALL, 33),      # 16 levels (epg 1, full groups), 9 columns
    (K2, O.TOY_N8192, (4, 3), TO_SMALL, 37), (ODD, N2049, (1, 16), TO_BIG, 1)],
    ids=["L1-9-b1", "L3-41-b33", "L5-2049-b37", "L15-41-b37", "L16-9-b33", "L3-9-b37", "L16-2049-b1"])
def test_product_geometry(src, dst, pair, target, count):
    """Edge digits and key words (edge_big_cts, edge_ksk) through ks_decompose_kernel + keyswitch_mfma_kernel at the cast
    key's (in_dim, out_size, level, base_log), against exact integers and the host loop."""
    f = _f()
    rng = np.random.default_rng([src.N, dst.N, dst.n, pair[0], pair[1], target, count])
    key, cts = edge_key(src, dst, pair, target, rng), edge_cts(src, dst, pair, target, rng, count)
    ck = _cast_key(src, dst, pair, target, key)
    got = ck.cast(cts, f.CAST_KEYSWITCHED)
    want = cast_exact(src, dst, pair, target, key, cts)
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and not len(bad), f"{len(bad)} of {want.size} words differ; first (row, word) {bad[:8].tolist()}"
    assert np.array_equal(got, f.cast_host(to_fhestr_params(dst), ck.cp, key, cts))
    info = ck.info()
    assert (info["in_dim"], info["out_dim"] + 1, info["last"]) == (src.k * src.N, want.shape[1], "lwes")
    ck.close()


# ---- cast_decompose_glwe_kernel ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,k", SHAPES, ids=[f"N{N}-k{k}" for N, k in SHAPES])
def test_fused_digits_from_glwes(N, k):
    """37 blocks that start 19 coefficients before the end of GLWE 0 (first > 0, two GLWEs: coefficients N - 19 .. N - 1, 0,
    1 .. 17) and 3 blocks around N / 2: the fused kernel's digit fragments are byte for byte those of ks_decompose_kernel on
    the extracted LWEs, and the keyswitched rows those of the unfused route and of exact integers."""
    f = _f()
    src, dst = _shape(k, N, f"SRC_N{N}_K{k}"), O.TOY_K1
    for pair in ((4, 3), (3, 5)):
        rng = np.random.default_rng([N, k, pair[0]])
        key = rng.integers(0, 2**64, size=k * N * pair[1] * (dst.n + 1), dtype=np.uint64)
        ck = _cast_key(src, dst, pair, TO_SMALL, key)
        for first, count in ((N - 19, 37), (N // 2 - 1, 3)):
            glwes = random_glwes(k, N, first, count, 5)
            want = cast_packed_exact(src, dst, pair, TO_SMALL, key, glwes, first, count)
            ck.set_fused(True)
            fused_rows, fused_digits = ck.cast_packed(glwes, count, first, f.CAST_KEYSWITCHED), ck.digits(glwes, count, first, packed=True)
            assert ck.info()["last"] == "fused"
            ck.set_fused(False)
            plain_rows, plain_digits = ck.cast_packed(glwes, count, first, f.CAST_KEYSWITCHED), ck.digits(glwes, count, first, packed=True)
            assert ck.info()["last"] == "extract"
            assert fused_digits.size == plain_digits.size == -(-count // 32) * -(-k * N // (2 * (16 // pair[1]))) * 1024
            assert np.array_equal(fused_digits, plain_digits), f"{(fused_digits != plain_digits).sum()} digit bytes differ"
            assert np.array_equal(fused_rows, plain_rows) and np.array_equal(fused_rows, want)
            if count == 37 and k * N <= 512:      # a fresh buffer: rows past the batch are still zero, as in the definition
                lwes = f.glwe_sample_extract_host(to_fhestr_params(src), glwes, count, first)
                assert np.array_equal(fused_digits, digit_fragments(lwes, k * N, *pair))
        ck.close()


@pytest.mark.parametrize("N,k", [(512, 3), (256, 1)], ids=["N512-k3", "N256-k1"])
def test_narrow_list_widened_on_the_device(N, k):
    """fhe_cast_narrow[_dev]: a source's narrow list -- its shape (k, N) is not the engine's -- goes up as stored, is widened by
    glwe_widen_kernel at the SOURCE's shape and keyswitched: word for word the exact cast of the host-widened GLWEs, for a
    range inside one stream and one that crosses into the next; host and device forms agree."""
    import torch
    f = _f()
    src, dst, pair = _shape(k, N, f"SRC_N{N}_K{k}"), O.TOY_K1, (4, 3)
    Ps = to_fhestr_params(src)
    rng = np.random.default_rng([N, k, 77])
    key = rng.integers(0, 2**64, size=k * N * pair[1] * (dst.n + 1), dtype=np.uint64)
    ck = _cast_key(src, dst, pair, TO_SMALL, key)
    held, bits = N + 40, 16
    narrow = f.glwe_narrow_host(Ps, rng.integers(0, 2**64, size=(2, k + 1, N), dtype=np.uint64), held, bits)
    wide = f.glwe_widen_host(Ps, narrow, held, bits)
    d_narrow = torch.from_numpy(narrow.view(np.int64)).to("cuda:0")
    for first, count in ((3, 37), (N - 19, 37), (0, held)):
        want = cast_packed_exact(src, dst, pair, TO_SMALL, key, wide, first, count)
        got = ck.cast_narrow(narrow, held, bits, count, first, f.CAST_KEYSWITCHED)
        assert np.array_equal(got, want)
        assert _engine(dst).narrow_info()["kernel"] == "widen" and ck.info()["last"] == "fused"
        d_rows = torch.zeros(want.shape, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        ck.cast_narrow(d_narrow, held, bits, count, first, f.CAST_KEYSWITCHED, d_out=d_rows.data_ptr())
        _engine(dst).synchronize()
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), want)
    with pytest.raises(f.FheError, match="asked of a list that holds"):
        ck.cast_narrow(narrow, held, bits, 2, held - 1, f.CAST_KEYSWITCHED)
    ck.close()


# The toy twins of 1_1 -> 2_2 keyswitch at (4, 6): the toy destination's nominal variance is 7.8e-11 of the torus, and the
# rounding of the mask at (4, 4), k N / 2 / (12 * 2^32) = 2.5e-9, would alone be 32 of its units -- 160 after a regrouping of
# two blocks (weights 1 and 2), above the toy budget of 99.6.  Six levels put it at 2^-48.
WIDE_PAIR = (4, 6)


# ---- the follow-up tables, on toy twins ---------------------------------------------------------------------------------------

class _Rig:
    """Two clients with library keys, the destination's server key resident on an engine of its own."""

    def __init__(self, src, dst, seed):
        f = _f()
        self.Ps, self.Pd = to_fhestr_params(src), to_fhestr_params(dst)
        self.ck_src, self.ck_dst = f.ClientKey(self.Ps, 0xCA570500 + seed), f.ClientKey(self.Pd, 0xCA570600 + seed)
        self.eng = f.Engine(self.Pd, 0)
        self.eng.load_keys(*self.ck_dst.gen_server_keys(threads=8))
        self.keys = {}

    def cast_key(self, target, pair=None, v_in=1.0):
        """v_in: what the test's source blocks carry (0 for the fresh encryptions of a toy source whose own lookups would be
        noisier than the toy destination's budget admits)."""
        if (target, pair) not in self.keys:
            cp, key = self.ck_src.gen_cast_key(self.ck_dst, target, pair, seed=0xCA57)
            self.keys[target, pair] = self.eng.cast_key(cp, key)
        self.keys[target, pair].set_input_noise(v_in)
        return self.keys[target, pair]


_RIGS = {}


def _rig(src, dst, seed=0):
    if (src.name, dst.name) not in _RIGS:
        _RIGS[src.name, dst.name] = _Rig(src, dst, seed)
    return _RIGS[src.name, dst.name]


@pytest.mark.parametrize("target", [TO_BIG, TO_SMALL], ids=["to_big", "to_small"])
def test_shift_two_table(target):
    """1_1 -> 2_2 on toy twins, the reference's table: 0 .. 3 and the overflow case 2 * 1 + 1 come out unchanged, carry 0."""
    f, rig = _f(), _rig(O.TOY_K2, O.TOY_K1)
    ck = rig.cast_key(target, WIDE_PAIR, v_in=0.0)
    assert ck.shift == 2 and ck.info()["shift"] == 2
    cts = rig.ck_src.encrypt([0, 1, 2, 3])
    with np.errstate(over="ignore"):
        cts = np.concatenate([cts, cts[1:2] * np.uint64(2) + cts[1:2]])
    for mode in (f.CAST_RAW, f.CAST_REFRESH):          # a shift always brings its table
        assert rig.ck_dst.decrypt(ck.cast(cts, mode)).tolist() == [0, 1, 2, 3, 3]


def test_shift_zero_both_modes_and_to_small():
    f, rig = _f(), _rig(O.TOY_K1, O.TOY_K1, seed=1)
    values = list(range(16))
    cts = rig.ck_src.encrypt(values)
    big = rig.cast_key(TO_BIG, (4, 4))
    raw, fresh = big.cast(cts, f.CAST_RAW), big.cast(cts, f.CAST_REFRESH)
    assert rig.ck_dst.decrypt(raw).tolist() == values and rig.ck_dst.decrypt(fresh).tolist() == values
    assert np.array_equal(raw, big.cast(cts, f.CAST_KEYSWITCHED)), "raw at shift 0 is the keyswitch alone, the reference's behaviour"
    assert not np.array_equal(raw, fresh)
    small = rig.cast_key(TO_SMALL)
    for mode in (f.CAST_RAW, f.CAST_REFRESH):
        assert rig.ck_dst.decrypt(small.cast(cts, mode)).tolist() == values
    assert rig.ck_src.decrypt(fresh).tolist() != values


def test_truncation_with_cast_prepare():
    """2_2 -> 1_1: Engine.cast_prepare on the source's engine, then the keyswitch: 12 gives (0, 0), 3 gives message 1, carry 1."""
    f = _f()
    back = _rig(O.TOY_K1, O.TOY_K2, seed=2)
    ck = back.cast_key(TO_BIG, (4, 4))
    assert ck.shift == -2
    src_eng = f.Engine(back.Ps, 0)                      # the SOURCE client's server key, on an engine of its own
    src_eng.load_keys(*back.ck_src.gen_server_keys(threads=8))
    prepared = src_eng.cast_prepare(back.ck_src.encrypt([0, 1, 2, 3, 12]), -2)
    got = back.ck_dst.decrypt(ck.cast(prepared, f.CAST_RAW)).tolist()
    assert [(v % 2, v // 2) for v in got] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 0)]
    with pytest.raises(f.FheError, match="negative shift"):
        src_eng.cast_prepare(prepared, 2)
    src_eng.close()


def test_device_forms_equal_the_host_forms():
    """fhe_cast_lwes_dev / fhe_cast_packed_dev on device tensors, enqueued on the engine's stream: the keyswitched rows are
    word for word those of the host forms (with `first` past the first GLWE, which the host form rebases), the refreshed
    blocks decrypt alike."""
    import torch
    f, rig = _f(), _rig(O.TOY_K1, O.TOY_K1, seed=1)
    ck = rig.cast_key(TO_SMALL)
    P, dev = rig.Ps, "cuda:0"
    values = [(3 * i + 1) % 16 for i in range(37)]
    cts = rig.ck_src.encrypt(values)
    glwes = random_glwes(P.k, P.N, P.N + 250, 37, 9)                    # blocks 506 .. 542 of three GLWEs
    d_cts = torch.from_numpy(cts.view(np.int64)).to(dev)
    d_glwes = torch.from_numpy(glwes.view(np.int64)).to(dev)
    d_rows = torch.zeros((37, P.n + 1), dtype=torch.int64, device=dev)
    d_out = torch.zeros((37, P.big_size), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ck.cast(d_cts, f.CAST_KEYSWITCHED, d_rows.data_ptr(), 37)
    rig.eng.synchronize()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), ck.cast(cts, f.CAST_KEYSWITCHED))
    ck.cast_packed(d_glwes, 37, P.N + 250, f.CAST_KEYSWITCHED, d_rows.data_ptr())
    rig.eng.synchronize()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), ck.cast_packed(glwes, 37, P.N + 250, f.CAST_KEYSWITCHED))
    ck.cast(d_cts, f.CAST_REFRESH, d_out.data_ptr(), 37)
    rig.eng.synchronize()
    assert rig.ck_dst.decrypt(d_out.cpu().numpy().view(np.uint64)).tolist() == values


# ---- strings ------------------------------------------------------------------------------------------------------------------

TEXT = b"the quick brown fox jumps over 1"       # 32 characters


def test_string_cast_same_set():
    """A 32-character string of client A as blocks, as a PackedString and as a NarrowString: cast to client B, decrypted by B,
    and matched against a string of B's own with eq."""
    f, rig = _f(), _rig(O.TOY_K1, O.TOY_K1, seed=1)
    P = rig.Ps
    ops = f.FheStringOps(rig.eng)
    blocks = rig.ck_src.encrypt(f.string_to_blocks(P, TEXT, 32))
    pp, pksk = rig.ck_src.gen_packing_key((7, 3), seed=3)          # three levels: packed blocks are operand-grade
    glwes = f.packing_keyswitch_host(P, pp, pksk, blocks)
    packed = f.PackedString(glwes, blocks.shape[0], 32)
    bits = f.narrow_default_bits(P, pp, operand=True)
    narrow = f.NarrowString(f.glwe_narrow_host(P, glwes, blocks.shape[0], bits), blocks.shape[0], 32, bits)
    mine = rig.ck_dst.encrypt(f.string_to_blocks(P, TEXT, 32))
    other = rig.ck_dst.encrypt(f.string_to_blocks(P, TEXT[:-1] + b"2", 32))
    for target in (TO_SMALL, TO_BIG):
        ck = rig.cast_key(target, None if target == TO_SMALL else (4, 4))
        for form in (blocks, packed, narrow):
            cast = ops.cast(form, ck, src_cap=32, pp=pp)
            assert cast.shape == blocks.shape
            assert f.blocks_to_string(P, rig.ck_dst.decrypt(cast)) == TEXT
            assert (ck.group, ck.v_in) == (1, 1.0), "the call's settings stay on the handle"
        # the narrow list went up as stored and was widened on the GPU, then decomposed straight from the GLWEs
        assert ck.info()["last"] == "fused" and rig.eng.narrow_info()["kernel"] == "widen" and rig.eng.narrow_info()["bits"] == bits
        with pytest.raises(f.FheError, match="a packed string carries its packing keyswitch's noise: pass pp"):
            ops.cast(packed, ck)
        assert rig.ck_dst.decrypt(ops.eq(cast, mine)).tolist() == [1] and rig.ck_dst.decrypt(ops.eq(cast, other)).tolist() == [0]
    ops.close()


def test_string_cast_widening_regroups():
    """1-bit blocks to 2-bit blocks (toy twins of 1_1 -> 2_2): two source blocks per destination block, one lookup each; the
    combined lookup input is at most 3 << 2 = 12 of 15 (tests/test_cast_host.py::test_regrouping_degrees)."""
    f, rig = _f(), _rig(O.TOY_K2, O.TOY_K1)
    ops = f.FheStringOps(rig.eng)
    text = b"Zm9v~\x01\xff "
    blocks = rig.ck_src.encrypt(f.string_to_blocks(rig.Ps, text, 8))
    assert blocks.shape[0] == 64
    for target in (TO_SMALL, TO_BIG):
        ck = rig.cast_key(target, WIDE_PAIR, v_in=0.0)
        cast = ops.cast(blocks, ck)
        assert cast.shape == (32, rig.Pd.big_size) and ck.group == 1, "regrouping is this call's, not the handle's"
        got = rig.ck_dst.decrypt(cast)
        assert got.max() < rig.Pd.msg_mod and f.blocks_to_string(rig.Pd, got) == text.rstrip(b"\0")
        assert rig.ck_dst.decrypt(ops.eq(cast, rig.ck_dst.encrypt(f.string_to_blocks(rig.Pd, text, 8)))).tolist() == [1]
        assert ck.cast(blocks[:3]).shape[0] == 3, "a later call on the key does not regroup"
    with pytest.raises(f.FheError, match="lookup input of up to 960"):       # four 1-bit blocks into a 4-bit block: 15 << 6
        wide = f.cast_default_params(rig.Ps, to_fhestr_params(O.TOY_N32768), TO_SMALL)
        key = np.zeros(f.cast_key_len(to_fhestr_params(O.TOY_N32768), wide), dtype=np.uint64)
        f.CastKey(_engine(O.TOY_N32768), wide, key).set_group(4)
    ops.close()


# ---- real parameter sets --------------------------------------------------------------------------------------------------------

_P22 = {}


def _p22_rig():
    """One PARAM_MESSAGE_2_CARRY_2 client B with its server key resident, shared by the two real-size cases."""
    if not _P22:
        f = _f()
        P = f.PARAM_MESSAGE_2_CARRY_2_KS_PBS
        ck = f.ClientKey(P, 0xCA570900)
        eng = f.Engine(P, 0)
        eng.load_keys(*ck.gen_server_keys(threads=16))
        _P22.update(P=P, ck=ck, eng=eng)
    return _P22


def test_p11_to_p22_to_big_reference_pair():
    """PARAM_MESSAGE_1_CARRY_1 -> PARAM_MESSAGE_2_CARRY_2 with the reference's key: TO_BIG, (1, 15), 378 MB; values 0 .. 3
    come out unchanged.  By fhe_cast_noise this key alone puts 1,126 of the destination's nominal variances on a block
    (k N * 15 digits of variance 1/2 under lwe_std = 7.07e-6: 5.8e-7 of the torus, the rounding of 1,536 mask words at 15
    bits 6e-8; V_pbs is 5.6e-10), 1,860 with a stored
    source block's own noise, against the PBS-input budget of 138 the plans use: the one-call cast, which ends in the table
    x >> 2, is refused even for fresh encryptions.  The reference runs the same two steps unguarded; they are taken here
    as the keyswitch alone and the destination's own lookup."""
    f, rig = _f(), _p22_rig()
    ck_src = f.ClientKey(f.PARAM_MESSAGE_1_CARRY_1_KS_PBS, 0xCA570901)
    cp, key = ck_src.gen_cast_key(rig["ck"], f.CAST_TO_BIG)
    assert (cp.base_log, cp.level) == (1, 15) and key.nbytes == 377_671_680
    ck = rig["eng"].cast_key(cp, key)
    del key
    assert ck.shift == 2
    cts = ck_src.encrypt([0, 1, 2, 3])
    nominal, budget, _ = f.cast_noise(rig["P"], cp, 0.0)
    print(f"P11 -> P22 TO_BIG (1, 15): {nominal:.1f} nominal variances from the key alone, budget {budget:.1f}")
    ck.set_input_noise(0.0)
    with pytest.raises(f.FheError, match="refused, a block keyswitched under the cast pair \\(1, 15\\)"):
        ck.cast(cts)
    rows = ck.cast(cts, f.CAST_KEYSWITCHED)
    lut_id, _ = rig["eng"].generate_lookup_table(lambda x: x >> 2)
    out = rig["eng"].apply_lookup_table(rows, np.full(4, lut_id, dtype=np.uint32))
    assert rig["ck"].decrypt(out).tolist() == [0, 1, 2, 3]
    ck.close()


def test_p22_to_p22_to_small_string_contains():
    f, rig = _f(), _p22_rig()
    P = rig["P"]
    alice = f.ClientKey(P, 0xCA570902)
    cp, key = alice.gen_cast_key(rig["ck"], f.CAST_TO_SMALL)
    assert (cp.base_log, cp.level) == (P.ks_base_log, P.ks_level)
    ck = rig["eng"].cast_key(cp, key)
    ops = f.FheStringOps(rig["eng"])
    stored = alice.encrypt(f.string_to_blocks(P, TEXT, 32))
    cast = ops.cast(stored, ck, src_cap=32)
    assert f.blocks_to_string(P, rig["ck"].decrypt(cast)) == TEXT
    assert rig["ck"].decrypt(ops.contains(cast, b"brown fox")).tolist() == [1]
    assert rig["ck"].decrypt(ops.contains(cast, b"brown cat")).tolist() == [0]
    ops.close()
    ck.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals():
    f, rig = _f(), _rig(O.TOY_K1, O.TOY_K1, seed=1)
    cts = rig.ck_src.encrypt([1, 2])
    # a raw block above the budget: one level of base 2 rounds the mask to a quarter of the torus
    noisy = rig.cast_key(TO_BIG, (1, 1))
    nominal, budget, _ = f.cast_noise(rig.Pd, noisy.cp)
    assert nominal > budget
    with pytest.raises(f.FheError, match="refused, a block keyswitched under the cast pair \\(1, 1\\)"):
        noisy.cast(cts, f.CAST_REFRESH)
    assert noisy.cast(cts, f.CAST_RAW).shape == cts.shape            # without a table nothing is judged: the reference's behaviour
    # narrowing a string
    back = _rig(O.TOY_K1, O.TOY_K2, seed=2)
    with pytest.raises(f.FheError, match="narrowing a string from 2 to 1 message bits"):
        f.FheStringOps(back.eng).cast(back.ck_src.encrypt(f.string_to_blocks(back.Ps, b"ab", 2)), back.cast_key(TO_BIG, (4, 4)))
    # a handle used on another engine
    other = f.Engine(rig.Pd, 0)
    with pytest.raises(f.FheError, match="resident on another engine"):
        f.FheStringOps(other).cast(cts, rig.cast_key(TO_SMALL))
    other.close()
    # blocks that are no whole groups, a key of the wrong size
    with pytest.raises(f.FheError, match="words are not the casting key"):
        f.CastKey(rig.eng, noisy.cp, np.zeros(5, dtype=np.uint64))


# ---- noise ----------------------------------------------------------------------------------------------------------------------

def _signed(x):
    return np.asarray(x, dtype=np.uint64).astype(np.int64).astype(np.float64)


@pytest.mark.parametrize("target", [TO_BIG, TO_SMALL], ids=["to_big", "to_small"])
def test_noise_matches_the_model(target):
    """tests/test_cast_host.py::test_noise_matches_the_model with the rows keyswitched on the GPU: S = 4096 blocks in one batch,
    the same model and the same margins (six standard errors of a mean, resp. of a variance estimate)."""
    f = _f()
    src = O.Params(16, 1, 1024, 10, 2, 4, 4, 4, 4, 1e-12, 1e-15, "TOY_SRC_N1024")
    dst = dataclasses.replace(O.TOY_K1, lwe_std=2.0**-20, name="TOY_K1_noisy_lwe")
    S, pair = 4096, (4, 4)
    Ps, Pd = to_fhestr_params(src), to_fhestr_params(dst)
    ck_src, ck_dst = f.ClientKey(Ps, 0xCA570300), f.ClientKey(Pd, 0xCA570301)
    cp, key = ck_src.gen_cast_key(ck_dst, target, pair, seed=17)
    cts = ck_src.encrypt(np.arange(S) % 16)
    ck = f.CastKey(_engine(dst), cp, key)
    rows = ck.cast(cts, f.CAST_KEYSWITCHED)
    big_src, _ = ck_src.secret_keys()
    big_dst, small_dst = ck_dst.secret_keys()
    sk_out = small_dst if target == TO_SMALL else big_dst
    with np.errstate(over="ignore"):
        diff = _signed((rows[:, -1] - rows[:, :-1] @ sk_out) - (cts[:, -1] - cts[:, :-1] @ big_src)) / 2.0**64
    model = f.cast_noise(Pd, cp, 0.0)[2]
    mean, var = diff.mean(), diff.var()
    print(f"cast noise on the GPU ({'small' if target else 'big'}): mean {mean:.3e}, variance {var:.4e}, model {model:.4e}, ratio {var / model:.4f}, "
          f"margin {6 * np.sqrt(2 / S):.4f}")
    assert abs(mean) <= 6 * np.sqrt(var / S)
    assert abs(var / model - 1) <= 6 * np.sqrt(2 / S)
    ck.close()
