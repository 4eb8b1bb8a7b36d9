"""A whole plan without noise (test infrastructure): the backend protocol of fhestr.distributed.ShardedPlanRunner -- the
one plan_oracle.OracleBackend, exact_plan.ExactBackend and fhestr.distributed.GpuBackend implement -- over a finalised plan's
exported levels (Plan.export_level / export_luts / info / level_info / level_rank_info), each ciphertext reduced to its
noise-free body: ONE torus phase per pool slot.

    pool         uint64 (slots, 1): with that shape exact_plan.gather_np / gather_int apply unchanged (big = 1), and
                 exact_plan.run_ranks steps several ranks,
    inputs       clear messages m, stored as m * delta,
    gather       the exported CSR, wrapping 64-bit integers (the exported constants are already scaled by delta),
    bootstrap    from first principles: idx = round(phase * 2N / 2^64) mod 2N; the result is body[idx] for idx < N and
                 -body[idx - N] otherwise, `body` the last N words of the exported accumulator, i.e. coefficient 0 of
                 X^-idx * accumulator.

What this sees: every value, every constant and every table of the plan, for the inputs given -- a range a builder asserted
wrongly (Circuit::lin's degree_override) lets the padding bit flip an answer here exactly as on the device.  What it does not
see: noise, and any kernel.  Nothing here reads csrc/ or calls the library beyond those exports."""
import numpy as np

U64 = np.uint64


def delta_of(params):
    return (1 << 63) // (params.msg_mod * params.carry_mod)


def gather_flat(pool, lv, jobs):
    """gather_np for pools of width 1, a level at a time: a wrapping running sum over the terms, differenced at the job
    boundaries (exact modulo 2^64).  tests/test_clear_plan.py pins it to gather_np and gather_int."""
    assert pool.shape[1] == 1
    jobs = np.asarray(jobs, dtype=np.int64)
    off = lv["off"].astype(np.int64)
    with np.errstate(over="ignore"):
        run = np.zeros(len(lv["src"]) + 1, dtype=U64)
        np.cumsum(pool[lv["src"].astype(np.int64), 0] * lv["coeff"].astype(np.int64).astype(U64), dtype=U64, out=run[1:])
        out = run[off[jobs + 1]] - run[off[jobs]] + lv["cst"][jobs]
    return out.reshape(len(jobs), 1)


class ClearBackend:
    """params: anything with N, msg_mod, carry_mod.  `levels` (CSR, constants, table ids, pool layout) and `bodies` (the
    last N words of every exported accumulator) are plain copies of the plan's exports: a test may edit them to build a
    deliberately wrong executor.  share: a dict that many backends intern their bodies in (read-only then) -- at
    N = 32768 a table is 256 KiB, and a sweep keeps thousands of plans over a few hundred distinct tables.
    Per run (reset() starts one; a fresh backend has started one):

        pools        every pool handed out, in order,
        inputs[l]    {job: gathered PBS-input phase} of level l, over all ranks that ran it,
        n_pbs        PBS inputs seen,
        off_centre   ... of them not a multiple of delta (no plan of the library has any: a Node::half share always
                     meets the constant that centres it before a lookup reads it),
        padding      ... of them with the padding bit set (legitimate: signed lookups, full boxes)."""

    def __init__(self, plan, params, gather=gather_flat, share=None):
        info = plan.info()
        self.plan, self.params, self.gather = plan, params, gather
        self.levels = [plan.export_level(l) for l in range(info["n_levels"] + 1)]
        self.N = params.N
        assert self.N & (self.N - 1) == 0
        luts = plan.export_luts()
        self.bodies = [self._body(luts[i], share) for i in range(len(luts))]
        self.delta = delta_of(params)
        self.reset()

    def _body(self, acc, share):
        body = np.array(acc[-self.N:], dtype=U64)
        if share is None:
            return body
        body.flags.writeable = False
        return share.setdefault(body.tobytes(), body)

    def reset(self):
        self.pools = []
        self.inputs = [{} for _ in self.levels[:-1]]
        self.n_pbs = self.off_centre = self.padding = 0

    def alloc_pool(self, slots):
        self.pools.append(np.zeros((slots, 1), dtype=U64))
        return self.pools[-1]

    def load_inputs(self, pool, inputs, n_inputs):
        with np.errstate(over="ignore"):
            pool[:n_inputs, 0] = np.asarray(inputs, dtype=U64).reshape(n_inputs) * U64(self.delta)

    def bootstrap(self, phase, lut_idx):
        """The noise-free programmable bootstrap of `phase` (uint64 array) on the tables lut_idx."""
        N = self.N
        log2n = N.bit_length() - 1
        idx = (((phase >> U64(62 - log2n)) + U64(1)) >> U64(1)).astype(np.int64) % (2 * N)     # round(phase * 2N / 2^64)
        val = np.zeros(len(phase), dtype=U64)
        for t in np.unique(lut_idx):
            at = lut_idx == t
            val[at] = self.bodies[t][idx[at] % N]
        with np.errstate(over="ignore"):
            return np.where(idx < N, val, U64(0) - val)

    def run_level(self, pool, level, rank):
        lv = self.levels[level]
        ri = self.plan.level_rank_info(level, rank)
        jobs = np.arange(ri["job_lo"], ri["job_hi"])
        if not len(jobs):
            return
        phase = self.gather(pool, lv, jobs)[:, 0]
        self.inputs[level].update(zip(jobs.tolist(), phase.tolist()))
        self.n_pbs += len(jobs)
        self.off_centre += int(np.count_nonzero(phase % U64(self.delta)))
        self.padding += int(np.count_nonzero(phase >> U64(63)))
        pool[lv["local_base"]: lv["local_base"] + len(jobs), 0] = self.bootstrap(phase, lv["lut"][jobs].astype(np.int64))

    def gather_outputs(self, pool, n_outputs):
        lv = self.levels[-1]
        return self.gather(pool, lv, np.arange(lv["jobs"]))[:, 0]


def decode(params, phases):
    """The messages modulo 2T (T = msg_mod * carry_mod: the padding bit included) of noise-free phases; every one of them
    must be a multiple of delta."""
    delta = delta_of(params)
    phases = np.asarray(phases, dtype=U64).reshape(-1)
    off = np.flatnonzero(phases % U64(delta))
    assert not len(off), f"{len(off)} of {len(phases)} phases are no multiple of delta: first at {off[:4].tolist()}, {hex(int(phases[off[0]]))}"
    return [int(v) for v in phases // U64(delta)]


def run_clear(backend, msgs):
    """World 1 through the product's own control flow, one fresh run: the decoded outputs."""
    from fhestr.distributed import ShardedPlanRunner
    backend.reset()
    return decode(backend.params, ShardedPlanRunner(backend.plan, 0, 1, backend).run(msgs))
