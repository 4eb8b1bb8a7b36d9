"""A whole plan in exact integers (test infrastructure): the backend protocol of fhestr.distributed.ShardedPlanRunner
(all of it but all_gather: several ranks are stepped in one process by run_ranks, which copies instead) over a finalised plan's exported levels (Plan.export_level / export_luts / level_rank_info), with

    gather       wrapping 64-bit integers, from the exported CSR (gather_np; gather_int is the same sum on Python
                 integers, one word at a time -- the definition; tests/test_exact_plan.py pins the one to the other),
    keyswitch    tests/exact_keyswitch.py: ExactKeyswitch,
    PBS          tests/exact_pbs.py: pbs_exact_batch / multi_bit_pbs_exact_batch over key terms (structured terms, or
                 limb_terms(bsk) for any key).

Under a structured bootstrapping key (exact_pbs.structured_bsk) a correct engine gives exactly these words for ANY
input ciphertexts, so every pool slot and every output word of a plan has one correct 64-bit value.

run_ranks steps all ranks of a plan in one process over per-rank pools, the all-gather done by the copies it stands
for; it is written against the backend protocol only, so the same loop drives ExactBackend, plan_oracle.OracleBackend
(numpy pools) and fhestr.distributed.GpuBackend (torch pools in HBM)."""
import numpy as np

from exact_keyswitch import ExactKeyswitch
from exact_pbs import multi_bit_pbs_exact_batch, pbs_exact_batch

U64 = np.uint64
M64 = (1 << 64) - 1


def gather_int(pool, lv, jobs):
    """out[r][e] = sum_t coeff[t] * pool[src[t]][e]  (+ cst[j] on the last word), mod 2^64, for j = jobs[r]: Python
    integers throughout, one multiplication at a time."""
    rows = {}
    out = []
    for j in jobs:
        acc = [0] * pool.shape[1]
        for t in range(int(lv["off"][j]), int(lv["off"][j + 1])):
            s, c = int(lv["src"][t]), int(lv["coeff"][t])
            if s not in rows:
                rows[s] = pool[s].tolist()
            acc = [a + c * w for a, w in zip(acc, rows[s])]
        acc[-1] += int(lv["cst"][j])
        out.append([v & M64 for v in acc])
    return np.array(out, dtype=U64).reshape(len(jobs), pool.shape[1])


def gather_np(pool, lv, jobs):
    """The same sum in wrapping uint64 arrays: a negative coefficient enters as its two's complement."""
    out = np.zeros((len(jobs), pool.shape[1]), dtype=U64)
    off, src = lv["off"].astype(np.int64), lv["src"].astype(np.int64)
    coeff = lv["coeff"].astype(np.int64).astype(U64)
    with np.errstate(over="ignore"):
        for r, j in enumerate(jobs):
            t0, t1 = off[j], off[j + 1]
            if t1 > t0:
                out[r] = (pool[src[t0:t1]] * coeff[t0:t1, None]).sum(axis=0, dtype=U64)
            out[r, -1] += lv["cst"][j]
    return out


class ExactBackend:
    """params: oracle Params of the engine's shape; ksk: the keyswitch key words; terms: the bootstrapping key as
    [(c, t)] (exact_pbs); grouping: multi-bit grouping factor, 0 for the classic PBS.  gather: gather_np or gather_int.
    `levels` (CSR, constants, table ids, pool layout) and `luts` are plain copies of the plan's exports: a test may
    edit them to build a deliberately wrong reference."""

    def __init__(self, plan, params, ksk, terms, grouping=0, gather=gather_np):
        n_levels = plan.info()["n_levels"]
        self.plan, self.params, self.terms, self.grouping, self.gather = plan, params, terms, grouping, gather
        self.levels = [plan.export_level(l) for l in range(n_levels + 1)]
        luts = plan.export_luts()
        self.luts = np.stack([luts[i] for i in range(len(luts))]) if luts else np.zeros((0, params.glwe_len), dtype=U64)
        self.keyswitch = ExactKeyswitch(params, ksk)
        self.big = params.big_size
        self.pools = []                                    # every pool handed out, in order: callers read them back

    def alloc_pool(self, slots):
        self.pools.append(np.zeros((slots, self.big), dtype=U64))
        return self.pools[-1]

    def load_inputs(self, pool, inputs, n_inputs):
        pool[:n_inputs] = np.asarray(inputs, dtype=U64).reshape(n_inputs, self.big)

    def pbs(self, small, lut_idx):
        if self.grouping:
            return multi_bit_pbs_exact_batch(self.params, self.grouping, self.terms, small, self.luts, lut_idx)
        return pbs_exact_batch(self.params, self.terms, small, self.luts, lut_idx)

    def run_level(self, pool, level, rank):
        lv = self.levels[level]
        ri = self.plan.level_rank_info(level, rank)
        jobs = list(range(ri["job_lo"], ri["job_hi"]))
        if not jobs:
            return
        staged = self.gather(pool, lv, jobs)
        idx = np.array([int(lv["lut"][j]) for j in jobs], dtype=np.int64)
        pool[lv["local_base"]: lv["local_base"] + len(jobs)] = self.pbs(self.keyswitch(staged), idx)

    def gather_outputs(self, pool, n_outputs):
        lv = self.levels[-1]
        return self.gather(pool, lv, list(range(lv["jobs"])))


def run_ranks(plan, inputs, backend, world=None, after_level=None):
    """All `world` ranks of `plan` in lockstep over one pool per rank (ShardedPlanRunner.run's loop, the collective
    replaced by copies: rank q's exported region -> slot q of every rank's receive region).  after_level(l, pools) is
    called once the level and its exchange are done.  Returns ([outputs of rank r], [pool of rank r])."""
    info = plan.info()
    world = info["world"] if world is None else world
    assert world == info["world"]
    pools = [backend.alloc_pool(info["pool_slots"]) for _ in range(world)]
    for pool in pools:
        backend.load_inputs(pool, inputs, info["n_inputs"])
    for l in range(info["n_levels"]):
        lv = plan.level_info(l)
        for r, pool in enumerate(pools):
            backend.run_level(pool, l, r)
        e = lv["e_max"]
        if world > 1 and e:
            for pool in pools:
                for q, src in enumerate(pools):
                    pool[lv["recv_base"] + q * e: lv["recv_base"] + (q + 1) * e] = src[lv["local_base"]: lv["local_base"] + e]
        if after_level:
            after_level(l, pools)
    return [backend.gather_outputs(pool, info["n_outputs"]) for pool in pools], pools


def run_exact(plan, inputs, backend):
    """World 1 through the product's own control flow (ShardedPlanRunner): (outputs, pool)."""
    from fhestr.distributed import ShardedPlanRunner
    out = ShardedPlanRunner(plan, 0, 1, backend).run(inputs)
    return out, backend.pools[-1]


def build_mixed_plan(plan, world=1, hints=False):
    """A hand-built plan holding the shapes the string and integer builders do not reliably produce together: a
    pbs_full_box node read through a negative coefficient (its half-delta share of the constant is subtracted), a signed
    PBS, a PBS of a trivial input (folded to a constant at build time), two jobs of one level that share a table, and
    two DISTINCT plan tables whose accumulators are identical (values 2T apart: Engine::lut_upload_dedup maps both to one
    resident copy).  Four inputs, five outputs, three levels.  Needs msg_mod * carry_mod >= 4."""
    T = plan.params.msg_mod * plan.params.carry_mod
    m = plan.params.msg_mod
    x = [plan.input(m - 1) for _ in range(4)]
    ident = plan.lut(lambda v: v % m)
    twin = plan.lut(lambda v: v % m + 2 * T)                  # another table, the same accumulator
    flip = plan.lut(lambda v: (T - 1 - v) % m)
    sgn = plan.lut(lambda v: int(v != 0))                      # odd: negacyclic for free
    assert len({ident, twin, flip, sgn}) == 4
    turn = iter(range(100))
    hint = (lambda: plan.set_owner_hint((3 * next(turn) + 1) % world)) if hints else (lambda: None)
    hint(); a = plan.pbs(plan.lin([(x[0], 1), (x[1], 1)]), ident)      # level 1: a and b share `ident`
    hint(); b = plan.pbs(x[2], ident)
    hint(); c = plan.pbs(x[3], flip)
    hint(); d = plan.pbs(plan.lin([(x[0], 1), (x[1], -1)]), sgn, signed=True)
    hint(); box = plan.pbs_full_box(plan.lin([(a, 1), (b, 1)]), all=False)          # level 2
    hint(); e = plan.pbs(plan.lin([(c, 1), (d, 1)], 1), twin)
    t = plan.pbs(plan.lin([], 2), flip)                        # trivial input: no job, a constant
    hint(); f = plan.pbs(plan.lin([(box, -1), (c, 1)], 1), flip)       # level 3: box through a negative coefficient
    hint(); g = plan.pbs(plan.lin([(box, 1), (t, 1)]), ident)
    for node in (f, g, e, plan.lin([(box, -1)], 1), t):
        plan.output(node)
    plan.finalize(world)
    return plan


def build_chain_plan(plan, world):
    """One two-step chain per rank, hinted onto it: level 1 is consumed by its own rank only, so it exports nothing
    (e_max = 0, no collective); level 2 feeds the outputs, one of them through a negative coefficient."""
    m = plan.params.msg_mod
    T = m * plan.params.carry_mod
    up = plan.lut(lambda v: (v + 1) % m)
    flip = plan.lut(lambda v: (T - 1 - v) % m)
    x = [plan.input(m - 1) for _ in range(world + 1)]
    ends = []
    for r in range(world):
        plan.set_owner_hint(r)
        a = plan.pbs(plan.lin([(x[r], 1), (x[r + 1], 1)]), up)
        a2 = plan.pbs(x[r], flip)
        ends.append(plan.pbs(plan.lin([(a, 1), (a2, 1)]), flip if r % 2 else up))
    plan.set_owner_hint(-1)
    for r, node in enumerate(ends):
        plan.output(node)
    plan.output(plan.lin([(ends[0], m - 1), (ends[-1], -1)], m - 1))
    plan.finalize(world)
    return plan
