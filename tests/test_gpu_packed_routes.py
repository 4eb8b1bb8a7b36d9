"""Engine.pack / unpack / narrow / unpack_narrow give the same words whichever side the input and the output lie on:
host array, host array + d_out, d_in alone, d_in + d_out, and a torch tensor in place of d_in.  The host -> host route
is the one the exact suites pin (test_gpu_packing_ks, test_gpu_glwe_extract, test_gpu_glwe_narrow); every other route
must reproduce it word for word and write nothing outside its output."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

LEVELS = {(256, 1): 2, (128, 2): 1}     # the level count the library instantiates per (N, k), as test_gpu_glwe_narrow has it
GUARD = 2**64 - 1
LEAD = 2                        # guard words in front of a device output: keeps it 8-byte aligned, not 256
K5 = next(p for p in O.TOY_SHAPES if p.name == "TOY_N256_K5")      # the smallest set test_gpu_packing_ks packs on, with its pair
K5_PAIR = (5, 2)


def _words(x):
    return np.asarray(x).view(np.uint64).reshape(-1)


def _all_routes(eng, run, src, what):
    """run(x, **kw): the engine call with its own arguments bound, x the host input, a device tensor or None (then d_in
    is among kw).  Returns the host -> host words after checking every other route against them."""
    import torch
    want = _words(run(src))
    d_src = torch.from_numpy(_words(src).view(np.int64).copy()).cuda()

    def on_device(x, **kw):
        d = torch.full((LEAD + want.size + 2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert run(x, d_out=d.data_ptr() + 8 * LEAD, **kw) is None
        eng.synchronize()
        h = d.cpu().numpy().view(np.uint64)
        assert (np.delete(h, np.s_[LEAD:LEAD + want.size]) == GUARD).all(), f"{what}: words outside the output were written"
        return h[LEAD:LEAD + want.size]

    torch.cuda.synchronize()
    routes = {
        "host + d_out": lambda: on_device(src),
        "d_in": lambda: _words(run(None, d_in=d_src.data_ptr())),
        "tensor": lambda: _words(run(d_src)),
        "d_in + d_out": lambda: on_device(None, d_in=d_src.data_ptr()),
        "tensor + d_out": lambda: on_device(d_src),
    }
    for route, go in routes.items():
        got = go()
        assert got.shape == want.shape, f"{what}, {route}: {got.size} words, host -> host gives {want.size}"
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{what}, {route}: {len(bad)} of {want.size} words differ from host -> host; first {bad[:12].tolist()}"
    return want


@pytest.mark.parametrize("N,k", [(256, 1), (128, 2)], ids=str)
def test_unpack_narrow_unpack_narrow(N, k):
    import fhestr
    eng = fhestr.Engine(fhestr.Params(8, k, N, 10, LEVELS[(N, k)], 4, 2, 4, 4, 1e-12, 1e-15, f"ROUTES_N{N}_K{k}"), 0)
    try:
        held, first, count, bits = N + 3, N - 2, 5, 13      # the rows span the boundary between the two GLWEs
        glwes = np.random.default_rng([N, k, 91]).integers(0, 2**64, size=(2, k + 1, N), dtype=np.uint64)
        rows = _all_routes(eng, lambda x, **kw: eng.unpack(x, count=count, first=first, refresh=False, **kw), glwes, f"unpack N={N} k={k}")
        assert rows.size == count * (k * N + 1)
        assert np.array_equal(rows, fhestr.glwe_sample_extract_host(eng.params, glwes, count, first).reshape(-1))
        narrow = _all_routes(eng, lambda x, **kw: eng.narrow(x, held, bits, **kw), glwes, f"narrow N={N} k={k}")
        assert narrow.size == fhestr.narrow_len(eng.params, held, bits)
        got = eng.narrow(d_in=_device(glwes).data_ptr(), held=held, bits=bits)
        assert isinstance(got, fhestr.NarrowString) and (got.count, got.bits, got.shape) == (held, bits, (1, narrow.size))
        rows = _all_routes(eng, lambda x, **kw: eng.unpack_narrow(x, held=held, bits=bits, count=count, first=first, refresh=False, **kw),
                           narrow, f"unpack_narrow N={N} k={k}")
        assert np.array_equal(rows, fhestr.narrow_sample_extract_host(eng.params, narrow, held, bits, count, first).reshape(-1))
    finally:
        eng.close()


def _device(words):
    import torch
    d = torch.from_numpy(_words(words).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d


def test_pack():
    import fhestr
    p = K5
    eng = fhestr.Engine(fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                                      p.lwe_std, p.glwe_std, p.name), 0)
    try:
        rng = np.random.default_rng([p.N, p.k, 92])
        eng.load_packing_key(K5_PAIR, rng.integers(0, 2**64, size=(p.k * p.N * K5_PAIR[1], p.k + 1, p.N), dtype=np.uint64))
        count = p.N + 3
        cts = rng.integers(0, 2**64, size=(count, p.k * p.N + 1), dtype=np.uint64)
        glwes = _all_routes(eng, lambda x, **kw: eng.pack(x, count=count, **kw), cts, "pack")
        assert glwes.size == 2 * (p.k + 1) * p.N
    finally:
        eng.close()
