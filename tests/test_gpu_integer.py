"""Integer plans on the GPU against the noise-free executor and Python integers: Plan.integer_op(eng, ...) through run_batch
on real encryptions, the first rows planted with the edge inputs of tests/integer_cases.py (0, 1, 2^w - 1, equal operands,
a + b = 2^w - 1, 2^w - 1 + 1, 0 - 1), decrypted and compared block for block with what tests/clear_plan.py gives for the same
clear inputs on an offline twin of the plan, and with the Python result.

Shapes: TOY_K1 and PARAM_MESSAGE_2_CARRY_2 (every name), TOY_N4096_L2 (1-bit blocks in a box of 32: the scan state in base
4), TOY_N8192 (3-bit blocks), TOY_N32768 and TOY_MULTI_BIT_N2048_G3's shape (the comparator block by block: two packed pairs
exceed their budgets).  Block counts 1, 3 (the smallest with a scanned carry state) and 5 (three scan steps, a trailing
unpacked comparator block); on PARAM_MESSAGE_2_CARRY_2 also 32, the FheUint64 shape.  64 instances where N <= 4096, 16 and
8 on the large polynomials: at most 8 x 18 lookups of N = 32768 per case."""
import numpy as np
import pytest

import conftest
import integer_cases as ic
import oracle as O
from clear_plan import ClearBackend, run_clear
from conftest import gpu_engine, keyset

pytestmark = pytest.mark.gpu

N4096 = next(p for p in O.TOY_SHAPES if p.name == "TOY_N4096_L2")
SHAPES = {"TOY_K1": O.TOY_K1, "P22": O.PARAM_MESSAGE_2_CARRY_2_KS_PBS, "TOY_N4096_L2": N4096, "TOY_N8192": O.TOY_N8192,
          "TOY_N32768": O.TOY_N32768, "TOY_MULTI_BIT_N2048_G3": O.TOY_MULTI_BIT_N2048_G3}
SOME = ("add", "sub", "scalar_add", "gt", "eq", "scalar_lt", "cmux")
CASES = [(s, name) for s in ("TOY_K1", "P22") for name in ic.NAMES] + [(s, name) for s in list(SHAPES)[2:] for name in SOME]
WIDE = ("add", "sub", "gt", "eq", "scalar_le", "scalar_sub")          # 32 blocks of PARAM_MESSAGE_2_CARRY_2


@pytest.fixture(scope="module", autouse=True)
def engines_opened_here():
    """Engines that this file is the first to open are closed when it is through (and leave conftest's cache)."""
    before = set(conftest._ENGINES)
    yield
    for key in set(conftest._ENGINES) - before:
        conftest._ENGINES.pop(key).close()


def _instances(p):
    return 64 if p.N <= 4096 else 16 if p.N <= 8192 else 8


def _scalars(name, n, bits, rng):
    """The scalars one name runs with: one in range; a comparison also one beyond the range, where there is room."""
    if name not in ic.SCALAR:
        return [0]
    w = n * bits
    top = (1 << w) - 1
    inside = int.from_bytes(rng.bytes(8), "little") & top
    if name in ic.BOOLEAN and w < 64:
        return [inside, (1 << w) + (inside | 1)]
    return [inside]


def _check(shape, name, n, scalars=None):
    import fhestr
    p = SHAPES[shape]
    ks = keyset(p)
    eng = gpu_engine(ks)
    P = eng.params
    M, T = P.msg_mod, P.msg_mod * P.carry_mod
    bits = M.bit_length() - 1
    rng = np.random.default_rng([list(SHAPES).index(shape), ic.NAMES.index(name), n])
    for scalar in scalars if scalars is not None else _scalars(name, n, bits, rng):
        plan = fhestr.Plan.integer_op(eng, name, n, scalar)
        twin = fhestr.Plan.integer_op(None, name, n, scalar, params=P)
        try:
            rows = ic.planted_rows(name, n, bits, T, rng, _instances(p), scalar)
            assert rows.shape == (_instances(p), plan.info()["n_inputs"])
            cts = ks.ck.encrypt_many(rows.reshape(-1)).reshape(rows.shape[0], rows.shape[1], P.big_size)
            out = plan.run_batch(cts)
            got = np.asarray(ks.ck.decrypt_many(out.reshape(-1, P.big_size))).reshape(rows.shape[0], -1)
            backend = ClearBackend(twin, P)
            for i, msgs in enumerate(rows.tolist()):
                want = ic.reference(name, n, bits, msgs, scalar)
                assert run_clear(backend, msgs) == want, (shape, name, n, scalar, msgs)
                assert got[i].tolist() == want, (shape, name, n, scalar, i, msgs, got[i].tolist(), want)
        finally:
            plan.close()
            twin.close()


@pytest.mark.parametrize("shape,name", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_blocks_1_3_5(shape, name):
    for n in (1, 3, 5):
        _check(shape, name, n)


@pytest.mark.parametrize("name", WIDE)
def test_p22_fheuint64_shape(name):
    """32 blocks of 2 bits: scalar_le against 2^64 - 1 (in range: the mask edge), scalar_sub of a full-width scalar."""
    scalars = {"scalar_le": [(1 << 64) - 1], "scalar_sub": [0xFEDCBA9876543211]}.get(name)
    _check("P22", name, 32, scalars)
