"""The batch sizes the library accepts, run: every batched entry point at and around the sizes where a grid dimension of
one of its launches passes 65535 / 65536, and at its documented limit (include/fhestr.h, "batch limits"), bit for bit
against exact integers.

Shape: TOY_K1 (N = 256, n = 16; rows of 257 words), so the largest batch here, 524280 LWEs, is 1.08 GB of input.

Inputs repeat with a PRIME period: 4099 distinct rows of edge_big_cts / edge_small_cts with a table chosen per row, the
exact references computed once for those 4099 rows (_case) and tiled.  Adjacent rows are distinct, and no index that
wraps at a power of two lands on an equal row: 65536 mod 4099 = 4051, 2^k mod 4099 != 0 for every k.  (The large batches
of tests/test_gpu_exact_rotation.py tile 64 rows: there a row index that wraps at any multiple of 64 goes unseen.)  Every
comparison is np.array_equal on whole ciphertexts.

  test_keyswitch_past_grid_y        Engine.keyswitch at 65535, 65536, 65537, 70001 LWEs on the matrix cores (ks_decompose_kernel
                                    has grid.y = count: two spans from 65537 on where the device reports 65536) and on the byte-plane
                                    kernel (FHESTR_KS_MFMA=0; grid.y = count / 8), against ExactKeyswitch
  test_keyswitch_limit              524280 accepted and exact on both; 524281 refused with the documented message, 5 LWEs right after exact
  test_lookup_paths_past_grid_y     KS + PBS, PBS alone and PBS -> KS at 65537 rows under a structured bootstrapping key, against
                                    pbs_exact_batch and ExactKeyswitch composed; then 5 rows on the same engine (grown buffers)
  test_plan_level_past_grid_y       eq (one shared pattern) and to_lower at capacity 32 over enough rows of a table that the widest
                                    level is one keyswitch and blind-rotation batch of more than 65536 rows; first 8, last 8 and the
                                    instances on either side of row 65536 of that level against ExactBackend, all of them against
                                    batches of 61
  test_pack_edge / test_ring_pack_edge / test_cast_edge
                                    65535 rows accepted, equal to the same rows in N-aligned calls of at most 1024, first and last
                                    GLWE (cast: rows) against the host reference; 65536 refused with the documented message, a small
                                    call right after answered correctly"""
import types

import numpy as np
import pytest

import oracle as O
from conftest import to_fhestr_params
from exact_cast import TO_SMALL, cast_exact
from exact_keyswitch import ExactKeyswitch, edge_big_cts
from exact_pbs import edge_small_cts, pbs_exact_batch
import exact_ring_packing as X
from test_gpu_exact_keyswitch import _assert_words
from test_gpu_exact_plan import _assert_outputs, _rig as _plan_rig
from test_gpu_exact_rotation import N_LUTS, _assert_exact, _Exact

pytestmark = pytest.mark.gpu

TOY = O.TOY_K1
PERIOD = 4099                                   # prime
KS_LIMIT = 524280
KS_REFUSAL = r"batch too large for one keyswitch launch \(max 524280 LWEs\)"


def test_period_is_prime_and_rows_are_distinct():
    assert all(PERIOD % d for d in range(2, 65)) and (1 << 16) % PERIOD == 4051
    c = _case()
    for rows in (c.big, c.small):
        assert len(np.unique(rows, axis=0)) == PERIOD
    for ref in (c.ks, c.ks_pbs, c.pbs, c.pbs_ks):
        assert len(np.unique(ref, axis=0)) == PERIOD          # a wrong row cannot hide behind an equal result


def _tile(B, first=0):
    """Which of the PERIOD distinct rows sits at each of B consecutive batch rows."""
    return (first + np.arange(B)) % PERIOD


_CASE = []


def _case():
    """The engines (one structured key: the matrix-core engine is test_gpu_exact_rotation's rig, the byte-plane engine holds
    the same keys), the PERIOD distinct inputs and their exact results on every path.  Built once, never written again."""
    if not _CASE:
        import fhestr
        rig = _Exact(TOY)
        c = types.SimpleNamespace(rig=rig, mfma=rig.eng)
        with pytest.MonkeyPatch.context() as mp:              # environment switches are read in Engine::create
            mp.setenv("FHESTR_KS_MFMA", "0")
            c.dot4 = fhestr.Engine(to_fhestr_params(TOY), 0)
        c.dot4.load_keys(rig.bsk.reshape(-1), rig.ksk)
        rng = np.random.default_rng([TOY.N, TOY.n, PERIOD])
        c.big = edge_big_cts(TOY, rng, PERIOD)
        c.small = edge_small_cts(TOY, rng, PERIOD)
        c.sel = rng.integers(0, N_LUTS, size=PERIOD)
        keyswitch = ExactKeyswitch(TOY, rig.ksk)
        c.ks = keyswitch(c.big)
        c.ks_pbs = pbs_exact_batch(TOY, rig.terms, c.ks, rig.luts, c.sel)
        c.pbs = pbs_exact_batch(TOY, rig.terms, c.small, rig.luts, c.sel)
        c.pbs_ks = keyswitch(c.pbs)
        for a in (c.big, c.small, c.sel, c.ks, c.ks_pbs, c.pbs, c.pbs_ks):
            a.setflags(write=False)
        _CASE.append(c)
    return _CASE[0]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _CASE:
        c.dot4.close()
        c.rig.close()
    _CASE.clear()


def _check_keyswitch(c, kernel, B, first=0):
    eng = getattr(c, kernel)
    idx = _tile(B, first)
    got = eng.keyswitch(c.big[idx])
    info = eng.keyswitch_info()
    print(f"batch-limits keyswitch {kernel} B={B}: {info}")
    assert info["kernel"] == kernel
    if kernel == "mfma":
        assert info["tile"] == min(8, 1 << max(0, (-(-B // 32) - 1).bit_length()))
    else:
        assert (info["tile"], info["chunks"]) == (8, TOY.k * TOY.N // 64)
    _assert_words(got, c.ks[idx], f"{kernel} B={B}")


# ---- 1: the keyswitch alone -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [65535, 65536, 65537, 70001], ids=lambda b: f"B{b}")
@pytest.mark.parametrize("kernel", ["mfma", "dot4"])
def test_keyswitch_past_grid_y(kernel, B):
    _check_keyswitch(_case(), kernel, B, first=B % 17)


@pytest.mark.parametrize("kernel", ["mfma", "dot4"])
def test_keyswitch_limit(kernel):
    import fhestr
    c = _case()
    _check_keyswitch(c, kernel, KS_LIMIT)
    with pytest.raises(fhestr.FheError, match=KS_REFUSAL):
        getattr(c, kernel).keyswitch(c.big[_tile(KS_LIMIT + 1)])
    _check_keyswitch(c, kernel, 5, first=PERIOD - 2)


# ---- 2: through the blind rotation ------------------------------------------------------------------------------------------

def test_lookup_paths_past_grid_y():
    c = _case()
    eng, ids = c.mfma, c.rig.ids
    for B, first in ((65537, 3), (5, 11)):                    # 5 after 65537: stale rows of the grown buffers
        idx = _tile(B, first)
        lut = ids[c.sel[idx]]
        got = eng.apply_lookup_table(c.big[idx], lut)
        assert eng.keyswitch_info()["kernel"] == "mfma"
        _assert_exact(got, c.ks_pbs[idx])
        _assert_exact(eng.pbs(c.small[idx], lut), c.pbs[idx])
        got = eng.apply_lookup_table_small_key(c.small[idx], lut)
        assert eng.keyswitch_info()["kernel"] == "mfma"
        _assert_words(got, c.pbs_ks[idx], f"PBS -> KS order B={B}")


# ---- 3: one level of a plan over many rows of a table -----------------------------------------------------------------------

def _plan_over_rows(rig, ops, op, cap, shared):
    """`op` at capacity `cap` over enough rows that its widest level exceeds 65536 rows; with `shared` the second operand is one
    pattern for all rows (it goes up once), else the plan is unary.  Returns how many of the instances held to exact have
    outputs of their own, and how many were held."""
    c = _case()
    plan = rig.string_op(op, cap, cap if shared else 0)
    widths = [plan.level_info(l)["jobs"] for l in range(plan.info()["n_levels"])]
    widest = max(widths)
    M = 65536 // widest + 1                                    # instances: the widest level is jobs x instances rows, job major
    assert widest * (M - 1) <= 65536 < widest * M
    print(f"batch-limits plan {op} capacity {cap}: level widths {widths}, {M} instances, widest level {widest * M} rows")
    blocks = cap * ops.bpc
    assert plan.info()["n_inputs"] == (2 if shared else 1) * blocks
    pat = c.big[_tile(blocks, PERIOD - blocks)] if shared else None
    rows = c.big[_tile(M * blocks)].reshape(M, blocks, -1)
    got = ops.op_many(op, rows, pat)
    at = 65536 % M                                             # row 65536 of the widest level is (job 65536 // M, instance `at`)
    pick = sorted({*range(8), *range(M - 8, M), (at - 1) % M, at})
    want = rig.exact_outputs(plan, np.stack([np.concatenate([rows[i], pat]) if shared else rows[i] for i in pick]))
    _assert_outputs(got[pick], want, f"{op} of {M} rows, instances {pick}")
    parts = np.concatenate([ops.op_many(op, rows[s:s + 61], pat) for s in range(0, M, 61)])
    _assert_outputs(got, parts, f"{op} of {M} rows against batches of 61")
    plan.close()
    return len(np.unique(want.reshape(len(pick), -1), axis=0)), len(pick)


def test_plan_level_past_grid_y():
    """eq at capacity 32 against one shared pattern, and to_lower at capacity 32: 64 jobs x 1025 instances = 65600 rows in the
    widest level of each.  Under the structured key the single output of eq takes very few values on these inputs (a table
    that is 0 off its first box forgets the rotation), so eq alone would not see rows that changed places; every instance
    of to_lower has outputs no other instance has, and that is asserted."""
    import fhestr
    with _plan_rig(TOY) as rig:
        ops = fhestr.FheStringOps(rig.eng)
        distinct, of = _plan_over_rows(rig, ops, "eq", 32, shared=True)
        print(f"batch-limits plan eq: {distinct} distinct outputs among {of} instances")
        distinct, of = _plan_over_rows(rig, ops, "to_lower", 32, shared=False)
        assert distinct == of, f"to_lower: only {distinct} of {of} instances have outputs of their own"


# ---- 4: the refusal edges of the packed paths ---------------------------------------------------------------------------------

EDGE = 65535


def _pack_edge(eng, host, refusal):
    """eng.pack at EDGE rows: against N-aligned calls of at most 1024 rows, first and last GLWE against host(rows); EDGE + 1
    refused; five rows answered correctly afterwards."""
    import fhestr
    c = _case()
    N = TOY.N
    rows = c.big[_tile(EDGE + 1, 7)]
    got = eng.pack(rows[:EDGE])
    assert got.shape == (-(-EDGE // N), TOY.k + 1, N)
    parts = np.concatenate([eng.pack(rows[s:min(s + 1024, EDGE)]) for s in range(0, EDGE, 1024)])
    assert np.array_equal(got, parts), f"{int((got != parts).any(axis=(1, 2)).sum())} of {len(got)} GLWEs differ from the calls of 1024 rows"
    last = (EDGE - 1) // N * N
    assert np.array_equal(got[:1], host(rows[:N])) and np.array_equal(got[-1:], host(rows[last:EDGE]))
    with pytest.raises(fhestr.FheError, match=refusal):
        eng.pack(rows)
    assert np.array_equal(eng.pack(rows[:5]), host(rows[:5]))


def test_pack_edge():
    import fhestr
    P = to_fhestr_params(TOY)
    pp = fhestr.packing_default_params(P)
    key = np.random.default_rng([TOY.N, 1]).integers(0, 2**64, size=fhestr.packing_key_len(P, pp), dtype=np.uint64)
    eng = fhestr.Engine(P, 0)
    try:
        eng.load_packing_key(pp, key)
        _pack_edge(eng, lambda rows: fhestr.packing_keyswitch_host(P, pp, key, rows), r"batch too large for one packing launch \(max 65535 LWEs\)")
        assert eng.packing_info()["ran"]
    finally:
        eng.close()


def test_ring_pack_edge():
    import fhestr
    P = to_fhestr_params(TOY)
    pair = fhestr.ring_packing_default_params(P)
    key = X.edge_key(TOY, pair, np.random.default_rng([TOY.N, 2]))
    eng = fhestr.Engine(P, 0)
    try:
        eng.load_ring_packing_key(pair, key)
        _pack_edge(eng, lambda rows: fhestr.ring_pack_host(P, pair, key, rows), r"batch too large for one ring packing call \(max 65535 LWEs\)")
        assert eng.ring_pack_info()["ran"] and not eng.packing_info()["ran"]
    finally:
        eng.close()


def test_cast_edge():
    import fhestr
    c = _case()
    P = to_fhestr_params(TOY)
    cp = fhestr.cast_default_params(P, P, fhestr.CAST_TO_SMALL)
    pair = (cp.base_log, cp.level)
    key = np.random.default_rng([TOY.N, 3]).integers(0, 2**64, size=fhestr.cast_key_len(P, cp), dtype=np.uint64)
    eng = fhestr.Engine(P, 0)
    try:
        ck = eng.cast_key(cp, key)
        rows = c.big[_tile(EDGE + 1, 9)]
        got = ck.cast(rows[:EDGE], fhestr.CAST_KEYSWITCHED)
        assert got.shape == (EDGE, TOY.n + 1) and ck.info()["last"] == "lwes"
        parts = np.concatenate([ck.cast(rows[s:min(s + 1024, EDGE)], fhestr.CAST_KEYSWITCHED) for s in range(0, EDGE, 1024)])
        _assert_words(got, parts, "cast of 65535 rows against calls of 1024")
        ends = np.r_[0:PERIOD, EDGE - 64:EDGE]                 # every distinct row once, and the last rows of the call
        _assert_words(got[ends], cast_exact(TOY, TOY, pair, TO_SMALL, key, rows[ends]), "cast of 65535 rows against exact")
        with pytest.raises(fhestr.FheError, match=r"cast: batch too large for one launch \(max 65535 blocks\)"):
            ck.cast(rows, fhestr.CAST_KEYSWITCHED)
        _assert_words(ck.cast(rows[:5], fhestr.CAST_KEYSWITCHED), fhestr.cast_host(P, cp, key, rows[:5]), "5 rows after the refusal")
        ck.close()
    finally:
        eng.close()
