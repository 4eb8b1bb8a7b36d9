"""Times of casting 1,024 PARAM_MESSAGE_2_CARRY_2 blocks to PARAM_MESSAGE_2_CARRY_2 (another client's key), device buffers,
host clock around a window of enqueued calls that ends in one synchronise -- 50 calls of the variants that hold a blind rotation
(0.4 s), 400 of the (1, 15) keyswitch, 4,000 of the 0.1 ms keyswitches (0.45 s) --; REPEATS rounds, the variants alternating
inside a round.
    python scripts/cast_timing.py [OUT]          (default: cast_timing.txt in the working directory; profiles/cast.txt keeps one run)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fhe-string-bounty_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

import fhestr as f

P = f.PARAM_MESSAGE_2_CARRY_2_KS_PBS
COUNT, REPEATS = 1024, 9
out_path = sys.argv[1] if len(sys.argv) > 1 else "cast_timing.txt"

t0 = time.time()
bob, alice = f.ClientKey(P, 0xCA570900), f.ClientKey(P, 0xCA570902)
eng = f.Engine(P, 0)
eng.load_keys(*bob.gen_server_keys(threads=16))
small = eng.cast_key(*alice.gen_cast_key(bob, f.CAST_TO_SMALL))
big = eng.cast_key(*alice.gen_cast_key(bob, f.CAST_TO_BIG))
print(f"keys ready after {time.time() - t0:.1f} s", flush=True)

dev = "cuda:0"
values = np.arange(COUNT) % 16
cts = alice.encrypt(values)
d_in = torch.from_numpy(cts.view(np.int64)).to(dev)
rng = np.random.default_rng(1)
d_glwes = torch.from_numpy(rng.integers(0, 2**63, size=(1, 2, 2048), dtype=np.int64)).to(dev)      # one GLWE holds 2,048 blocks
d_out = torch.empty((COUNT, P.big_size), dtype=torch.int64, device=dev)
d_mid = torch.empty((COUNT, P.big_size), dtype=torch.int64, device=dev)
ident, _ = eng.generate_lookup_table(lambda x: x)
d_idx = torch.full((COUNT,), ident, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def level():            # what Engine::refresh_rows_dev enqueues: one ks_pbs level with the identity table
    eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), COUNT)


def to_small():
    small.cast(d_in, f.CAST_REFRESH, d_out.data_ptr(), COUNT)


def to_big_two_steps():  # the (1, 15) keyswitch alone, then the destination's own level: the one-call form is refused at this set
    big.cast(d_in, f.CAST_KEYSWITCHED, d_mid.data_ptr(), COUNT)
    eng.apply_lookup_table_dev(d_mid.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), COUNT)


def to_big_keyswitch():
    big.cast(d_in, f.CAST_KEYSWITCHED, d_mid.data_ptr(), COUNT)


def packed(fused):
    def run():
        small.cast_packed(d_glwes, COUNT, 0, f.CAST_REFRESH, d_out.data_ptr())
    run.fused = fused
    return run


def packed_ks(fused):      # the keyswitch of a packed batch alone: digits (+ extraction) + product, no rotation
    def run():
        small.cast_packed(d_glwes, COUNT, 0, f.CAST_KEYSWITCHED, d_mid.data_ptr())
    run.fused = fused
    return run


def small_ks():
    small.cast(d_in, f.CAST_KEYSWITCHED, d_mid.data_ptr(), COUNT)


# (name, call, calls per timed window)
variants = [("level (ks_pbs, identity table)", level, 50), ("TO_SMALL", to_small, 50), ("TO_BIG (1,15) keyswitch + level", to_big_two_steps, 50),
            ("TO_BIG (1,15) keyswitch alone", to_big_keyswitch, 400), ("packed, fused digits", packed(True), 50), ("packed, extraction + digits", packed(False), 50),
            ("keyswitch alone, from LWE rows", small_ks, 4000), ("keyswitch alone, packed, fused", packed_ks(True), 4000),
            ("keyswitch alone, packed, extraction", packed_ks(False), 4000)]

# results must agree before they are timed: TO_SMALL decrypts, packed fused == packed unfused
to_small()
eng.synchronize()
assert bob.decrypt(d_out.cpu().numpy().view(np.uint64)).tolist() == values.tolist()
outs = []
for fused in (True, False):
    small.set_fused(fused)
    packed(fused)()
    eng.synchronize()
    outs.append(d_out.cpu().numpy().copy())
same = bool(np.array_equal(outs[0], outs[1]))

times = {name: [] for name, _, _ in variants}
for r in range(REPEATS + 1):
    for name, fn, calls in variants:
        if hasattr(fn, "fused"):
            small.set_fused(fn.fused)
        eng.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        eng.synchronize()
        if r:                                   # round 0 warms every shape up
            times[name].append((time.perf_counter() - t) / calls * 1e3)

with open(out_path, "w") as fh:
    fh.write(f"1,024 blocks, PARAM_MESSAGE_2_CARRY_2 -> PARAM_MESSAGE_2_CARRY_2, kernel revision {f.kernel_revision()}; ms per call: median [min .. max] of {REPEATS} "
             f"windows (host clock, one synchronise per window, variants alternating)\n")
    for name, _, calls in variants:
        v = sorted(times[name])
        fh.write(f"{name:36s} {v[len(v) // 2]:8.3f}  [{v[0]:.3f} .. {v[-1]:.3f}]   {calls} calls per window\n")
    fh.write(f"packed fused == packed unfused, word for word: {same}\n")
    fh.write(f"last keyswitch launch of the engine: {eng.keyswitch_info()}\n")
print(open(out_path).read())
