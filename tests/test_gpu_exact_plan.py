"""Whole plan execution against exact integers (tests/exact_plan.py), bit for bit.

Under a structured bootstrapping key (exact_pbs.structured_bsk) a correct KS + PBS is bit exact for ANY input
ciphertext, so every output word -- and every pool slot -- of a plan has one correct 64-bit value, however many levels
deep.  Inputs are not encryptions: the structured rows of edge_big_cts and uniformly random full-range words, all
distinct; nothing is decrypted; every comparison is np.array_equal on whole ciphertexts, mask and body.

Which test reaches what (csrc/circuit.cpp, csrc/lwe_kernels.hip.h):
    run_host_parts, one part      test_plan_run_every_op, test_plan_run_other_shapes      lincomb_kernel
    run_host_parts, two parts     test_two_operand_entry_points                           lincomb_kernel
    run_batch_host                test_run_batch, test_buffer_growth_and_reuse            lincomb_batch_kernel, lwe_restride_kernel
    run_batch_host with `shared`  test_shared_operand                                     lwe_restride_kernel with in_inst = 0
    run_batch_dev                 test_device_arrays_and_guard_rows, test_compact_and_seeded_inputs
    run_level_rank, gather_outputs  test_sharded_on_one_gpu (whole pool of every rank after every level)
Operation names come from the library's own source (_dispatch_names: the table of string plan names, the integer dispatch);
the `_reference` suffix and the `replace:F:C` forms, which the names' parser takes apart, are listed by hand in VARIANTS.
The pool of run_host_parts and of the batch paths lives inside the plan and cannot be read from Python without a new
entry point, so those paths are compared on their outputs; the sharded path is compared slot by slot.

The shape with k = 2 (the n = 8 twin of PARAM_MESSAGE_2_CARRY_1) has carry_mod < msg_mod: the string and integer builders
refuse it, so it runs the hand-built plans."""
import os
import re

import numpy as np
import pytest

import oracle as O
from conftest import ROOT
from exact_keyswitch import ExactKeyswitch, edge_big_cts
from exact_plan import ExactBackend, build_chain_plan, build_mixed_plan, run_exact, run_ranks
from test_gpu_exact_rotation import N1024, N2048, N_LUTS, P22, _assert_exact, _Exact

pytestmark = pytest.mark.gpu

MB_G2 = O.TOY_MULTI_BIT_N2048                     # N = 2048, n = 12, grouping factor 2
SENTINEL = 0x5A5AA5A5C3C33C3C                     # below 2^63: the same number as int64 and as uint64


class _Rig(_Exact):
    """_Exact (fresh engine, structured bootstrapping key, uniformly random keyswitch key) plus the plan-level reference."""

    def __enter__(self):
        self.plans = []
        return self

    def __exit__(self, *exc):
        for plan in self.plans:                 # a plan frees device memory through its engine: never after the engine
            plan.close()
        self.close()

    def _keep(self, plan):
        self.plans.append(plan)
        return plan

    def string_op(self, *args):
        import fhestr
        return self._keep(fhestr.Plan.string_op(self.eng, *args))

    def integer_op(self, *args):
        import fhestr
        return self._keep(fhestr.Plan.integer_op(self.eng, *args))

    def new_plan(self):
        import fhestr
        return self._keep(fhestr.Plan(self.eng))

    @property
    def P(self):
        return self.eng.params

    def backend(self, plan):
        return ExactBackend(plan, self.p, self.ksk, self.terms, grouping=self.G)

    def exact(self, plan, inputs):
        """(outputs, pool) of one instance."""
        return run_exact(plan, inputs, self.backend(plan))

    def exact_outputs(self, plan, inputs):
        """[instances, n_outputs, big] for inputs [instances, n_inputs, big]."""
        b = self.backend(plan)
        return np.stack([run_exact(plan, x, b)[0] for x in inputs])

    def cts(self, *shape):
        """All-distinct input ciphertexts [*shape, big]: edge rows first, uniformly random words after them."""
        return edge_big_cts(self.p, self.rng, int(np.prod(shape))).reshape(*shape, self.p.big_size)


def _rig(p, G=0, seed=0):
    return _Rig(p, G, 0, seed)


def _assert_outputs(got, want, plan_name):
    """got / want [instances, n_outputs, big] (or [n_outputs, big]): names output job, instance and differing words."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (plan_name, got.shape, want.shape)
    got, want = got.reshape(-1, *got.shape[-2:]), want.reshape(-1, *want.shape[-2:])
    bad = np.argwhere((got != want).any(axis=2))
    if len(bad):
        first = "; ".join(f"output level, job {j}, instance {i}: {int((got[i, j] != want[i, j]).sum())} words" for i, j in bad[:6])
        raise AssertionError(f"{plan_name}: {len(bad)} of {got.shape[0] * got.shape[1]} output ciphertexts differ from exact "
                             f"({int((got != want).sum())} words) -- {first}")


def _slot_names(plan, rank):
    """{pool slot: "level l, job j"} for what rank `rank` holds: its own jobs and every rank's exported ones."""
    info = plan.info()
    names = {s: f"input {s}" for s in range(info["n_inputs"])}
    for l in range(info["n_levels"]):
        lv = plan.level_info(l)
        for r in range(info["world"]):
            ri = plan.level_rank_info(l, r)
            for i, j in enumerate(range(ri["job_lo"], ri["job_hi"])):
                if r == rank:
                    names[lv["local_base"] + i] = f"level {l}, job {j}"
                if i < ri["n_export"]:
                    names[lv["recv_base"] + r * lv["e_max"] + i] = f"level {l}, job {j} (received from rank {r})"
    return names


def _assert_pool(got, want, plan, rank, when):
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        names = _slot_names(plan, rank)
        first = "; ".join(f"slot {s} ({names.get(s, 'no job of this rank: must stay zero')}), instance 0: {int((got[s] != want[s]).sum())} words"
                          for s in bad[:6])
        raise AssertionError(f"rank {rank} {when}: {len(bad)} of {len(want)} pool slots differ from exact "
                             f"({int((got != want).sum())} words) -- {first}")


# ---- the operation names the library accepts, read from its dispatch code --------------------------------------------------

EXPECTED_STRING_BASES = {"eq", "ne", "lt", "le", "gt", "ge", "eq_ignore_case", "starts_with", "ends_with", "contains", "find", "rfind", "strip_prefix",
                       "strip_suffix", "concat", "repeat", "replace", "to_upper", "to_lower", "trim_start", "trim_end", "strip", "trim", "len", "is_empty"}


def _dispatch_names():
    """(string bases, integer names).  The string bases are read from the table of plan names (csrc/str_op_name.cpp, one
    Row(name, family, forms, params, bare, ...) per line): the rows that build without parameters (bare), outside the
    families this file does not run -- matches_clear takes a pattern text, which b"ab" is not, and runs bit for bit on
    this rig in tests/test_gpu_regex.py; the split family has its own tests.  The integer names are every name that
    build_integer_op compares with."""
    csrc = os.path.join(ROOT, "fhe-string-bounty_amd", "csrc")
    with open(os.path.join(csrc, "str_op_name.cpp")) as f:
        s = f.read()
    rows = re.findall(r'^ *Row\("(\w+)", (\w+), ([\w |]+), (\d+), (true|false)[,)]', s[s.index("const Row TABLE[] = {"):s.index("\n};")], re.M)
    assert len(rows) == s.count("Row(\""), "a row of the table that this test cannot read"
    strings = sorted(name for name, family, _, _, bare in rows if bare == "true" and family not in ("MATCHES", "SPLIT"))
    assert set(strings) == EXPECTED_STRING_BASES and len(strings) == 25, sorted(set(strings) ^ EXPECTED_STRING_BASES)
    with open(os.path.join(csrc, "fhe_integer.cpp")) as f:
        s = f.read()
    s = s[s.index("int build_integer_op("):]
    plain, scalar = set(re.findall(r'\bop == "(\w+)"', s)), set(re.findall(r'\bbase == "(\w+)"', s))
    return strings, sorted(plain | scalar | {"scalar_" + n for n in scalar})


STRING_BASES, INTEGER_NAMES = _dispatch_names()
CLEAR = {"repeat": b"\x02", "replace": b"abxy"}      # repeat_clear: the count; replace_clear: from || to


NO_ENCRYPTED_FORM = {"repeat"}                       # the count of a repetition is clear: the only form that must not build
# what the dispatch accepts beyond base names: the reference's circuit shape (no packed comparison, no full-box reduction)
# and the general replace with a pattern capacity / length and an output capacity
VARIANTS = [("eq_reference", 2, None), ("contains_reference", 2, None), ("lt_reference", 2, None), ("find_reference_clear", 0, b"ab"),
            ("ne_reference_clear", 0, b"ab"), ("replace:1:3", 2, None), ("replace_clear:1:3", 0, b"axy"), ("replace_clear:0:3", 0, b"x")]


def _string_plans(rig, a_cap=2, b_cap=2):
    """[(name, plan)]: every string base with an encrypted second operand and with a clear one, then VARIANTS.  Exactly the
    forms of NO_ENCRYPTED_FORM are refused; anything else that stops building is an error here, not a smaller run."""
    import fhestr
    plans, refused = [], set()
    for base in STRING_BASES:
        for name, clear in ((base, None), (base + "_clear", CLEAR.get(base, b"ab"))):
            try:
                plans.append((name, rig.string_op(name, a_cap, 0 if clear else b_cap, clear)))
            except fhestr.FheError:
                refused.add(name)
    assert refused == NO_ENCRYPTED_FORM, f"forms that do not build: {sorted(refused)}, expected {sorted(NO_ENCRYPTED_FORM)}"
    for name, cap, clear in VARIANTS:
        plans.append((name, rig.string_op(name, a_cap, cap, clear)))
    return plans


def test_dispatch_names_are_what_the_library_accepts():
    """The names read from the source are complete enough to be the library's set: each builds, a foreign one does not."""
    import fhestr
    assert len(STRING_BASES) >= 25 and {"eq", "find", "replace", "to_lower", "repeat", "trim"} <= set(STRING_BASES)
    assert len(INTEGER_NAMES) >= 19 and {"cmux", "add", "scalar_add", "scalar_le", "carry_extract"} <= set(INTEGER_NAMES)
    with _rig(O.TOY_K1) as rig:
        for name in ("no_such_op", "eq_", "Eq"):
            with pytest.raises(fhestr.FheError, match="unknown string op"):
                rig.string_op(name, 2, 2)
            with pytest.raises(fhestr.FheError, match="unknown integer op"):
                rig.integer_op(name, 2)
        assert len(_string_plans(rig)) == 2 * len(STRING_BASES) - len(NO_ENCRYPTED_FORM) + len(VARIANTS)
        for name in INTEGER_NAMES:
            rig.integer_op(name, 2, 3)


# ---- Plan.run: host buffers, run_host_parts ---------------------------------------------------------------------------------

def _check_run(rig, name, plan):
    inputs = rig.cts(plan.info()["n_inputs"])
    want, _ = rig.exact(plan, inputs)
    _assert_outputs(plan.run(inputs), want, name)


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_plan_run_every_op(p):
    """Every string_op and integer_op name of the dispatch code, small capacities, and the hand-built plan."""
    with _rig(p) as rig:
        for name, plan in _string_plans(rig):
            _check_run(rig, name, plan)
            plan.close()
        for name in INTEGER_NAMES:
            _check_run(rig, "integer " + name, rig.integer_op(name, 3, 6))
        _check_run(rig, "mixed", build_mixed_plan(rig.new_plan()))


# (shape, grouping, string ops, integer ops); the radix comparisons on every shape: tests/test_gpu_integer.py
OTHER = [(N1024, 0, (), ()), (MB_G2, 2, ("eq", "lt", "find"), ("add", "cmux")), (P22, 0, ("le",), ("le", "add"))]


@pytest.mark.parametrize("p,G,ops,int_ops", OTHER, ids=[o[0].name for o in OTHER])
def test_plan_run_other_shapes(p, G, ops, int_ops):
    """k = 2 (hand-built plans only: carry_mod < msg_mod), multi-bit with grouping 2, and the real n = 742 of
    PARAM_MESSAGE_2_CARRY_2 under a structured key (two small plans: its exact reference walks 742 steps per level)."""
    with _rig(p, G) as rig:
        _check_run(rig, "mixed", build_mixed_plan(rig.new_plan()))
        for op in ops:
            _check_run(rig, op, rig.string_op(op, 2, 2))
        for op in int_ops:
            _check_run(rig, "integer " + op, rig.integer_op(op, 2))
        if p is not P22:
            inputs = rig.cts(3, 4)
            plan = build_mixed_plan(rig.new_plan())
            _assert_outputs(plan.run_batch(inputs), rig.exact_outputs(plan, inputs), "mixed, batch of 3")


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_two_operand_entry_points(p):
    """FheStringOps._binary: two host arrays (run_host_parts with two parts) and a clear pattern, against Plan.run on the
    concatenated inputs and against exact."""
    import fhestr
    with _rig(p) as rig:
        ops = fhestr.FheStringOps(rig.eng)
        both = rig.cts(5 * ops.bpc)                     # one draw: no ciphertext of b is one of a
        a, b = both[:3 * ops.bpc], both[3 * ops.bpc:]
        assert len(np.unique(both, axis=0)) == len(both)
        for op in ("eq", "find", "le", "ends_with"):
            plan = rig.string_op(op, 3, 2)
            want, _ = rig.exact(plan, both)
            _assert_outputs(plan.run(both), want, op)
            _assert_outputs(ops._binary(op, a, b), want, op + " (two operands)")
            plan = rig.string_op(op + "_clear", 3, 0, b"Ab")
            want, _ = rig.exact(plan, a)
            _assert_outputs(plan.run(a), want, op + "_clear")
            _assert_outputs(ops._binary(op, a, b"Ab"), want, op + " (clear pattern)")


# ---- many instances in one pass -------------------------------------------------------------------------------------------

def _crossing_count(plan, limit=None):
    """Smallest instance count for which jobs x instances of the plan's widest level exceeds `limit`; by default the
    device's compute units (256 on an MI355X): choose_rotate_path (csrc/blind_rotate.hip) then takes the variant that shares a
    CU between two LWEs.  The count follows the device, so the case cannot go stale against that threshold."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    limit = cus if limit is None else limit
    widest = max(plan.level_info(l)["jobs"] for l in range(plan.info()["n_levels"]))
    return limit // widest + 1, widest, limit


@pytest.mark.parametrize("p,op", [(N2048, "eq"), (N2048, "find"), (O.TOY_K1, "contains")], ids=["N2048-eq", "N2048-find", "TOY_K1-contains"])
def test_run_batch(p, op):
    """Plan.run_batch at 1, 2, 3, 17 instances and at the first count for which the widest level holds more than 256
    rows (N = 2048: that level's blind rotation then runs two LWEs per CU); every instance has its own inputs; instance i
    against Plan.run of instance i and against exact."""
    with _rig(p) as rig:
        plan = rig.string_op(op, 3, 2)
        cross, widest, cus = _crossing_count(plan)
        assert cus >= 256 and widest * (cross - 1) <= cus < widest * cross
        n_in = plan.info()["n_inputs"]
        inputs = rig.cts(max(cross, 17), n_in)
        assert len(np.unique(inputs.reshape(-1, rig.p.big_size), axis=0)) == inputs.shape[0] * n_in        # no two ciphertexts alike
        want = rig.exact_outputs(plan, inputs)
        single = np.stack([plan.run(x) for x in inputs[:17]])
        _assert_outputs(single, want[:17], f"{op}, Plan.run per instance")
        for count in (1, 2, 3, 17, cross):
            _assert_outputs(plan.run_batch(inputs[:count]), want[:count], f"{op}, batch of {count}")
        # another window of the same rows: instance 0 of this call is not instance 0 of the last one
        _assert_outputs(plan.run_batch(inputs[5:8]), want[5:8], f"{op}, batch of 3 from instance 5")


def test_run_batch_multi_bit_fused_kernel():
    """Multi-bit, grouping 2: the widest level at the last instance count that still fits multibit_combine_max = 64 rows (the
    combined prepass, as in test_plan_run_other_shapes) and at the first one beyond it, where choose_rotate_path takes the
    fused kernel; narrower levels of the same pass stay in the prepass."""
    with _rig(MB_G2, 2) as rig:
        plan = rig.string_op("find", 3, 2)
        cross, widest, limit = _crossing_count(plan, 64)
        assert limit == 64 and widest * (cross - 1) <= 64 < widest * cross
        assert min(plan.level_info(l)["jobs"] for l in range(plan.info()["n_levels"])) * cross <= 64
        inputs = rig.cts(cross, plan.info()["n_inputs"])
        want = rig.exact_outputs(plan, inputs)
        for count in (cross - 1, cross) if cross > 1 else (cross,):
            _assert_outputs(plan.run_batch(inputs[:count]), want[:count], f"find, multi-bit, batch of {count}")


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_shared_operand(p):
    """run_batch_host with `shared` (FheStringOps.op_many / eq_many: one pattern against many rows): the pattern is copied
    to every instance by lwe_restride_kernel with in_inst = 0.  The pattern differs from every row, rows differ from each other."""
    import fhestr
    with _rig(p) as rig:
        ops = fhestr.FheStringOps(rig.eng)
        for count in (1, 3, 17):
            drawn = rig.cts(count * 3 * ops.bpc + 2 * ops.bpc)          # one draw: the pattern shares no ciphertext with a row
            assert len(np.unique(drawn, axis=0)) == len(drawn)
            pat, rows = drawn[:2 * ops.bpc], drawn[2 * ops.bpc:].reshape(count, 3 * ops.bpc, -1)
            full = np.stack([np.concatenate([r, pat]) for r in rows])
            for op in ("eq", "find"):
                plan = rig.string_op(op, 3, 2)
                want = rig.exact_outputs(plan, full)
                _assert_outputs(ops.op_many(op, rows, pat), want, f"{op} of {count} rows against one pattern")
                _assert_outputs(plan.run_batch(full), want, f"{op}, batch of {count}")
                if op == "eq":
                    _assert_outputs(ops.eq_many(rows, pat)[:, None], want, f"eq_many of {count} rows")
                plan.close()
        rows = rig.cts(3, 3 * ops.bpc)                                             # no second operand at all
        plan = rig.string_op("to_upper", 3)
        _assert_outputs(ops.op_many("to_upper", rows), rig.exact_outputs(plan, rows), "to_upper of 3 rows")


def _run_dev_guarded(rig, plan, inputs, name, d_in=None):
    """run_batch_dev (run_dev for one instance) into a sentinel-filled buffer with guard rows on both sides."""
    import torch
    info = plan.info()
    count, n_out, big = len(inputs), info["n_outputs"], rig.p.big_size
    guard = 3
    rows = count * n_out
    d_out = torch.full((rows + 2 * guard, big), SENTINEL, dtype=torch.int64, device="cuda")
    if d_in is None:
        d_in = torch.from_numpy(np.ascontiguousarray(inputs).view(np.int64)).cuda()
    torch.cuda.synchronize()                           # torch's stream is not ordered with the engine's
    out_ptr = d_out.data_ptr() + guard * big * 8
    if count == 1:
        plan.run_dev(d_in.data_ptr(), out_ptr)
    else:
        plan.run_batch_dev(d_in.data_ptr(), out_ptr, count)
    rig.eng.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    assert (got[:guard] == SENTINEL).all() and (got[guard + rows:] == SENTINEL).all(), f"{name}: rows outside the outputs were written"
    _assert_outputs(got[guard: guard + rows].reshape(count, n_out, big), rig.exact_outputs(plan, inputs), name)
    assert not (got[guard: guard + rows] == SENTINEL).all(axis=1).any()


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_device_arrays_and_guard_rows(p):
    """run_dev and run_batch_dev on torch arrays: every output word overwritten and exact, nothing outside
    [0, instances x n_outputs) rows touched."""
    with _rig(p) as rig:
        for name, plan in (("to_lower", rig.string_op("to_lower", 2)), ("find", rig.string_op("find", 3, 2)),
                           ("mixed", build_mixed_plan(rig.new_plan()))):
            for count in (1, 2, 5):
                _run_dev_guarded(rig, plan, rig.cts(count, plan.info()["n_inputs"]), f"{name}, {count} on device arrays")


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_compact_and_seeded_inputs(p):
    """A compact public-key list expanded by the GPU straight into run_dev's input array, and a seeded batch expanded by
    expand_seeded_lwe, against exact on the host expansions."""
    import fhestr
    import torch
    from fhestr import wire
    with _rig(p) as rig:
        plan = rig.string_op("eq", 3, 2)
        n_in, big = plan.info()["n_inputs"], rig.p.big_size
        clist = rig.rng.integers(0, 2**64, size=fhestr.compact_list_len(rig.P, n_in), dtype=np.uint64)
        d_in = torch.zeros((n_in, big), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rig.eng.expand_compact_list(clist, n_in, d_out=d_in.data_ptr())
        host = fhestr.expand_compact_host(rig.P, clist, n_in)
        _run_dev_guarded(rig, plan, host[None], "eq on a compact list", d_in=d_in)
        count = 3
        seeds = rig.rng.integers(0, 256, size=(count * n_in, 16), dtype=np.uint8)
        bodies = rig.rng.integers(0, 2**64, size=count * n_in, dtype=np.uint64)
        d_in = torch.zeros((count * n_in, big), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rig.eng.expand_seeded_lwe(seeds, bodies, d_out=d_in.data_ptr())
        host = wire.decompress_lwe_batch(rig.p.k * rig.p.N, seeds, bodies).reshape(count, n_in, big)
        _run_dev_guarded(rig, plan, host, "eq on a seeded batch of 3", d_in=d_in)


# ---- sharded execution, all ranks on one GPU ---------------------------------------------------------------------------------

def _sharded_plans(rig, world):
    """(name, plan for `world`, the same circuit finalised for world 1 or None).  eq and contains reduce one slice of the
    characters per rank (csrc/str_ops.h, owner_for): for world > 1 that is another circuit than world 1's, with
    other words.  The others are one circuit in every world, so their outputs must be world 1's word for word."""
    yield "eq", rig.string_op("eq", 8, 8, None, world), None
    yield "contains", rig.string_op("contains", 8, 2, None, world), None
    yield "find", rig.string_op("find", 3, 2, None, world), rig.string_op("find", 3, 2)
    yield "to_lower", rig.string_op("to_lower", 3, 0, None, world), rig.string_op("to_lower", 3)
    yield "replace_clear", rig.string_op("replace_clear", 4, 0, b"abxy", world), rig.string_op("replace_clear", 4, 0, b"abxy")
    yield "mixed with owner hints", build_mixed_plan(rig.new_plan(), world, hints=True), build_mixed_plan(rig.new_plan())
    yield "chain (level 1 exports nothing)", build_chain_plan(rig.new_plan(), world), None


@pytest.mark.parametrize("world", [2, 4, 8], ids=lambda w: f"world{w}")
@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_sharded_on_one_gpu(p, world):
    """ShardedPlanRunner's backend GpuBackend(reuse_pool=False), all ranks in one process over separate pools in HBM, the
    gather done by copies: after EVERY level each rank's whole pool equals the exact executor's pool for that rank --
    slots it neither owns nor receives are still zero -- and all ranks end with the same outputs."""
    import torch
    from fhestr.distributed import GpuBackend
    with _rig(p) as rig:
        try:
            for name, plan, single in _sharded_plans(rig, world):
                inputs = rig.cts(plan.info()["n_inputs"])
                snaps = {}
                want, _ = run_ranks(plan, inputs, rig.backend(plan), after_level=lambda l, pools: snaps.__setitem__(l, [q.copy() for q in pools]))
                if name.startswith("chain"):
                    assert plan.level_info(0)["e_max"] == 0 and plan.level_info(1)["e_max"] > 0

                def compare(l, pools):
                    for r, pool in enumerate(pools):
                        _assert_pool(pool.cpu().numpy().view(np.uint64), snaps[l][r], plan, r, f"of {name} (world {world}) after level {l}")

                got, _ = run_ranks(plan, inputs, GpuBackend(plan, torch.device("cuda", 0), reuse_pool=False), after_level=compare)
                for r in range(world):
                    _assert_outputs(got[r], want[r], f"{name}, world {world}, rank {r}")
                    assert np.array_equal(got[r], got[0])
                if single is not None:
                    assert (single.info()["n_pbs"], single.info()["n_levels"]) == (plan.info()["n_pbs"], plan.info()["n_levels"])
                    _assert_outputs(got[0], rig.exact(single, inputs)[0], f"{name}, world {world}, against world 1")
                    _assert_outputs(single.run(inputs), got[0], f"{name}, Plan.run of world 1 against world {world}")
        finally:
            rig.eng.set_stream(None)


# ---- state carried between calls --------------------------------------------------------------------------------------------

def _many_tables_plan(plan, count):
    """`count` jobs in one level, each on a table of its own."""
    m = plan.params.msg_mod
    T = m * plan.params.carry_mod
    x = [plan.input(m - 1), plan.input(m - 1)]
    ids = set()
    for i in range(count):
        lut = plan.lut(lambda v, i=i: ((i + 1) >> (v % 8) & 1) + (v == i % T))
        ids.add(lut)
        plan.output(plan.pbs(x[i % 2], lut))
    assert len(ids) == count
    plan.finalize(1)
    return plan


def _lut_count(eng):
    import ctypes
    import fhestr
    n = ctypes.c_uint32()
    assert fhestr.lib().fhe_lut_count(eng.handle, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_table_array_growth_between_plans(p):
    """Plan A, then a plan B with enough new tables that the engine's resident table array is reallocated, then A again."""
    with _rig(p) as rig:
        a = rig.string_op("find", 3, 2)
        xa = rig.cts(a.info()["n_inputs"])
        want_a, _ = rig.exact(a, xa)
        _assert_outputs(a.run(xa), want_a, "plan A")
        before = _lut_count(rig.eng)
        assert before <= 64                                    # the array's first capacity (Engine::lut_upload)
        b = _many_tables_plan(rig.new_plan(), 150)
        assert _lut_count(rig.eng) >= before + 150 > 128            # past two doublings of the array
        xb = rig.cts(2)
        want_b, _ = rig.exact(b, xb)
        _assert_outputs(b.run(xb), want_b, "plan B (table array grown)")
        _assert_outputs(a.run(xa), want_a, "plan A after the table array grew")
        _assert_outputs(a.run_batch(np.stack([xa, xa[::-1]])), rig.exact_outputs(a, np.stack([xa, xa[::-1]])), "plan A, batch, after the growth")


@pytest.mark.parametrize("mode", [2, 1], ids=lambda m: f"pipeline{m}")
def test_plan_right_after_pipelined_calls(mode):
    """Several apply_lookup_table_dev calls under set_pipeline(mode), then -- no synchronise in between, the mode still
    set -- a plan through the host path and through the batch path.  Every call and both plan runs exact."""
    import torch
    B, calls = 96, 3
    with _rig(N2048) as rig:
        keyswitch = ExactKeyswitch(rig.p, rig.ksk)
        big = [rig.cts(B) for _ in range(calls)]
        sel = [(np.arange(B) + c) % N_LUTS for c in range(calls)]
        wants = [rig.reference(keyswitch(b), s) for b, s in zip(big, sel)]
        plan = rig.string_op("find", 3, 2)
        x = rig.cts(3, plan.info()["n_inputs"])
        want_plan = rig.exact_outputs(plan, x)
        ins = [torch.from_numpy(b.view(np.int64)).cuda() for b in big]
        idx = [torch.from_numpy(rig.ids[s].astype(np.int32)).cuda() for s in sel]
        outs = [torch.zeros_like(t) for t in ins + ins]           # one buffer per call of either round
        torch.cuda.synchronize()
        rig.eng.set_pipeline(mode)
        try:
            for i, o, t in zip(ins, outs[:calls], idx):
                rig.eng.apply_lookup_table_dev(i.data_ptr(), t.data_ptr(), o.data_ptr(), B)
            got_single = plan.run(x[0])
            for i, o, t in zip(ins, outs[calls:], idx):
                rig.eng.apply_lookup_table_dev(i.data_ptr(), t.data_ptr(), o.data_ptr(), B)
            got_batch = plan.run_batch(x)
            rig.eng.synchronize()
        finally:
            rig.eng.set_pipeline(0)
        for o, want in zip(outs, wants + wants):
            _assert_exact(o.cpu().numpy().view(np.uint64), want)
        _assert_outputs(got_single, want_plan[0], f"find after pipelined calls (mode {mode})")
        _assert_outputs(got_batch, want_plan, f"find, batch of 3, after pipelined calls (mode {mode})")


@pytest.mark.parametrize("p", [N2048, O.TOY_K1], ids=lambda p: p.name)
def test_buffer_growth_and_reuse(p):
    """One plan at 2, then 9, then 2 instances (the batch buffers grow, then are reused with a smaller stride), and two
    plans of one engine run alternately through every entry point."""
    with _rig(p) as rig:
        a = rig.string_op("find", 3, 2)
        b = rig.string_op("to_lower", 2)
        xa, xb = rig.cts(9, a.info()["n_inputs"]), rig.cts(9, b.info()["n_inputs"])
        wa, wb = rig.exact_outputs(a, xa), rig.exact_outputs(b, xb)
        for lo, hi in ((0, 2), (0, 9), (7, 9), (3, 4)):
            _assert_outputs(a.run_batch(xa[lo:hi]), wa[lo:hi], f"find, instances {lo}..{hi}")
        for turn in range(2):
            for name, plan, x, w in (("find", a, xa, wa), ("to_lower", b, xb, wb)):
                _assert_outputs(plan.run(x[turn]), w[turn], f"{name}, alternating, turn {turn}")
                _assert_outputs(plan.run_batch(x[turn: turn + 4]), w[turn: turn + 4], f"{name}, batch, alternating, turn {turn}")
