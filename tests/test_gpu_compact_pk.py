"""Compact public-key ciphertext lists on the GPU (csrc/compact_kernels.hip.h): the device expansion is bit-identical to
fhe_compact_expand_host through both entry points, and a list encrypted with the PUBLIC key runs through FheString
operations and KS + PBS without an expanded ciphertext ever crossing PCIe.  The CPU side is tests/test_compact_pk.py."""
import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params

pytestmark = pytest.mark.gpu

GUARD = 0x6A5D39EAB7C4F012


def _f():
    import fhestr
    return fhestr


_ENG = {}


def _engine(params):
    """Key-less engine (the expansion needs none), cached per parameter set."""
    if params.name not in _ENG:
        _ENG[params.name] = _f().Engine(to_fhestr_params(params), 0)
    return _ENG[params.name]


def _dev_zeros(words):
    import torch
    t = torch.zeros(words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()          # torch's stream is not the engine's: order it before any engine call
    return t


def _to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    return t.cpu().numpy().view(np.uint64)


CASES = [(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, c) for c in (1, 1024, 2048, 2049, 5000)] + \
        [(O.PARAM_MESSAGE_2_CARRY_1_KS_PBS, c) for c in (3, 2049)] + \
        [(O.TOY_K1, c) for c in (1, 255, 256, 257, 700)] + \
        [(O.PARAM_MESSAGE_4_CARRY_4_KS_PBS, c) for c in (1, 37, 2048)]


@pytest.mark.parametrize("params,count", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_device_expansion_is_bit_identical_to_the_host(params, count):
    """Random containers (the expansion does not care what the words mean).  Host-list entry point into device memory with
    a guard word behind the last row, the same into host memory, and the _dev entry point from a resident list."""
    f = _f()
    P = to_fhestr_params(params)
    eng = _engine(params)
    big = P.big_size
    rng = np.random.default_rng(count + P.N)
    clist = rng.integers(0, 2**64, size=f.compact_list_len(P, count), dtype=np.uint64)
    want = f.expand_compact_host(P, clist, count)
    # host list -> device rows; one guard word behind the last row, and one row of slack in front to catch a stray store
    d = _dev_zeros(big + count * big + 1)
    d[:big] = GUARD
    d[-1] = GUARD
    import torch
    torch.cuda.synchronize()
    assert eng.expand_compact_list(clist, count, d_out=d.data_ptr() + 8 * big) is None
    got = _host(d)
    assert np.all(got[:big] == np.uint64(GUARD)) and got[-1] == np.uint64(GUARD)
    assert np.array_equal(got[big:-1].reshape(count, big), want)
    del d, got
    # host list -> host rows
    if count * big * 8 <= 64 << 20:
        assert np.array_equal(eng.expand_compact_list(clist, count), want)
    # resident list -> device rows, no synchronisation inside
    d_list = _to_dev(clist)
    d = _dev_zeros(count * big + 1)
    d[-1] = GUARD
    torch.cuda.synchronize()
    eng.expand_compact_list(None, count, d_out=d.data_ptr(), d_list=d_list.data_ptr())
    eng.synchronize()
    got = _host(d)
    assert got[-1] == np.uint64(GUARD)
    assert np.array_equal(got[:-1].reshape(count, big), want)


def test_device_expansion_refuses_other_dimensions():
    f = _f()
    eng = _engine(O.PARAM_MESSAGE_1_CARRY_1_KS_PBS)        # k = 3, N = 512
    with pytest.raises(f.FheError, match="do not hold|power-of-two"):
        eng.expand_compact_list(np.zeros(1537, dtype=np.uint64), 1)
    import ctypes as C
    buf = np.zeros(4096, dtype=np.uint64)
    assert f.lib().fhe_engine_expand_compact_list(eng.handle, buf.ctypes.data_as(C.c_void_p), 1, None, buf.ctypes.data_as(C.c_void_p)) != 0
    assert "power-of-two" in f.lib().fhe_last_error().decode()


@pytest.fixture(scope="module")
def p22_public():
    """PARAM_MESSAGE_2_CARRY_2: client key, its compact public key, and an engine whose server keys were generated on the device."""
    f = _f()
    P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
    ck = f.ClientKey(P, 0xC11E47)
    pk = ck.compact_public_key(0x9B11C)
    eng = f.Engine(P, 0)
    g, s = ck.secret_keys()
    eng.generate_keys(g, s, 0x5E4F)
    yield P, ck, pk, eng
    eng.close()


def _run_resident(plan, d_in_ptr, P):
    info = plan.info()
    d_out = _dev_zeros(info["n_outputs"] * P.big_size)
    plan.run_dev(d_in_ptr, d_out.data_ptr())
    plan.engine.synchronize()
    return _host(d_out).reshape(info["n_outputs"], P.big_size)


def test_strings_encrypted_with_the_public_key(p22_public):
    """Two strings go out as ONE compact list under the public key, are expanded in HBM, and eq / contains / to_lower run
    on the resident ciphertexts; the client key decrypts what Python's bytes give."""
    f = _f()
    P, ck, pk, eng = p22_public
    bpc = f.blocks_per_char(P)
    a, b, a_cap, b_cap = b"Hello, World", b"World", 16, 8
    for second, seed in ((b, 1), (b"world", 2), (a, 3)):
        cap2 = a_cap if second == a else b_cap
        blocks = np.concatenate([f.string_to_blocks(P, a, a_cap), f.string_to_blocks(P, second, cap2)])
        clist = pk.encrypt(blocks, seed)
        assert clist.size == 2048 + blocks.size          # one bin: what crosses PCIe
        d_in = _dev_zeros(blocks.size * P.big_size)
        eng.expand_compact_list(clist, blocks.size, d_out=d_in.data_ptr())
        for op, want in (("eq", a == second), ("contains", second in a)):
            plan = f.Plan.string_op(eng, op, a_cap, cap2)
            assert plan.info()["n_inputs"] == blocks.size
            got = ck.decrypt(_run_resident(plan, d_in.data_ptr(), P))
            assert list(got) == [int(want)], (op, second)
            plan.close()
        plan = f.Plan.string_op(eng, "to_lower", a_cap)      # the first a_cap * bpc rows are the first string
        assert plan.info()["n_inputs"] == a_cap * bpc
        got = f.blocks_to_string(P, ck.decrypt(_run_resident(plan, d_in.data_ptr(), P)))
        assert got == a.lower()
        plan.close()


def test_ks_pbs_of_every_message_value(p22_public):
    f = _f()
    import torch
    P, ck, pk, eng = p22_public
    M = P.msg_mod * P.carry_mod
    table = lambda x: (5 * x + 3) % M
    lut_id, _ = eng.generate_lookup_table(table)
    msgs = np.tile(np.arange(P.msg_mod, dtype=np.uint64), 16)
    d_in = _dev_zeros(msgs.size * P.big_size)
    d_out = _dev_zeros(msgs.size * P.big_size)
    d_idx = torch.full((msgs.size,), lut_id, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.expand_compact_list(pk.encrypt(msgs, 77), msgs.size, d_out=d_in.data_ptr())
    eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), msgs.size)
    eng.synchronize()
    got = ck.decrypt(_host(d_out).reshape(msgs.size, P.big_size))
    assert np.array_equal(got, np.array([table(int(m)) for m in msgs]))


def test_compact_list_through_the_wire(p22_public):
    """What a tfhe-rs-shaped public-key client sends: shortint CompactCiphertextList bytes -> read -> GPU expansion -> decrypt."""
    f = _f()
    from fhestr import wire
    P, ck, pk, eng = p22_public
    msgs = np.random.default_rng(5).integers(0, P.msg_mod, size=2100, dtype=np.uint64)
    data = wire.write_shortint_compact_list(P, pk.encrypt(msgs, 99), msgs.size)
    assert len(data) == 8 + 8 * (2 * 2048 + 2100) + 8 + 8 + 24 + 24 + 4 + 8
    clist, count, meta, _, used = wire.read_shortint_compact_list(P, data)
    assert count == msgs.size and used == len(data) and meta == wire.compact_meta(P)
    cts = eng.expand_compact_list(clist, count)
    assert np.array_equal(cts, f.expand_compact_host(P, clist, count))
    assert np.array_equal(ck.decrypt(cts), msgs.astype(np.int64))
