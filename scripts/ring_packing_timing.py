#!/usr/bin/env python3
"""Times ring packing (csrc/ring_packing_kernels.hip.h) beside what it stands next to, and records its noise:

  * PARAM_MESSAGE_2_CARRY_2: fhe_engine_ring_pack_lwes_dev for 256 and 1,024 LWEs, and the matrix packing keyswitch
    (fhe_engine_pack_lwes_dev) for the same batches on the same visit;
  * PARAM_MESSAGE_4_CARRY_4: 2,048 LWEs, beside the device-to-host copy of the 537 MB they occupy as LWEs;
  * key bytes and client key-generation time for both sets;
  * measured / modelled variance of the host reference on the two toy shapes of tests/test_ring_packing.py.

HIP events on the stream the engine launches on, warm; medians over --reps calls.  Writes a text report.

    python scripts/ring_packing_timing.py [--out profiles/ring_packing.txt] [--reps 50]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("fhe-string-bounty_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fhestr  # noqa: E402


def timed(stream, fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t):
    med, lo, hi = t
    return f"{med * 1e3:10.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_packing.txt"))
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    stream = torch.cuda.current_stream()
    lines = [f"ring packing, kernels {fhestr.kernel_revision()}",
             f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"HIP events, median (min .. max) of {args.reps} calls after 5 warm-up calls"]

    # ---- PARAM_MESSAGE_2_CARRY_2: both routes ----
    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    msgs = np.arange(1024) % (P.msg_mod * P.carry_mod)
    d_cts = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_glwe = torch.zeros((1, P.k + 1, P.N), dtype=torch.int64).cuda()
    t0 = time.perf_counter()
    pair, rkey = ck.gen_ring_packing_key(seed=fhestr.random_seed())
    ring_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    pp, mkey = ck.gen_packing_key(seed=fhestr.random_seed())
    matrix_s = time.perf_counter() - t0
    lines += [f"{P.name}",
              f"  ring key, pair {pair}: {rkey.nbytes} bytes as 64-bit words, {rkey.nbytes * 4} bytes resident as transformed planes; CPU generation {ring_s:.2f} s",
              f"  matrix key, pair {pp}: {mkey.nbytes} bytes; CPU generation {matrix_s:.2f} s"]
    for name, load in (("ring", lambda e: e.load_ring_packing_key(pair, rkey)), ("matrix", lambda e: e.load_packing_key(pp, mkey))):
        eng = fhestr.Engine(P, 0)
        load(eng)
        eng.set_stream(stream.cuda_stream)
        for count in (256, 1024):
            t = timed(stream, lambda: eng.pack(d_in=d_cts.data_ptr(), count=count, d_out=d_glwe.data_ptr()), args.reps)
            stream.synchronize()
            ok = np.array_equal(ck.decrypt_packed(d_glwe.cpu().numpy().view(np.uint64), count), msgs[:count])
            extra = ""
            if name == "ring":
                info = eng.ring_pack_info()
                extra = f"   {info['keyswitches']} automorphism keyswitches, {info['launches']} launches, {info['scratch_bytes']} scratch bytes;"
            lines.append(f"  {name:6s} pack_lwes_dev {count:5d} LWEs: {fmt(t)}{extra} decrypts: {ok}")
        eng.close()
    ck.close()

    # ---- PARAM_MESSAGE_4_CARRY_4: the set the matrix route refuses ----
    P = fhestr.PARAM_MESSAGE_4_CARRY_4_KS_PBS
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    count = 2048
    msgs = np.arange(count) % (P.msg_mod * P.carry_mod)
    d_cts = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_glwe = torch.zeros((1, P.k + 1, P.N), dtype=torch.int64).cuda()
    t0 = time.perf_counter()
    pair, rkey = ck.gen_ring_packing_key(seed=fhestr.random_seed())
    ring_s = time.perf_counter() - t0
    eng = fhestr.Engine(P, 0)
    eng.load_ring_packing_key(pair, rkey)
    eng.set_stream(stream.cuda_stream)
    t = timed(stream, lambda: eng.pack(d_in=d_cts.data_ptr(), count=count, d_out=d_glwe.data_ptr()), args.reps, warmup=2)
    stream.synchronize()
    info = eng.ring_pack_info()
    ok = np.array_equal(ck.decrypt_packed(d_glwe.cpu().numpy().view(np.uint64), count), msgs)
    host = torch.empty(d_cts.shape, dtype=torch.int64).pin_memory()
    copy = timed(stream, lambda: host.copy_(d_cts, non_blocking=True), args.reps)
    lines += [f"{P.name}",
              f"  ring key, pair {pair}: {rkey.nbytes} bytes as 64-bit words, {rkey.nbytes * 4} bytes resident as transformed planes; CPU generation {ring_s:.2f} s",
              f"  ring   pack_lwes_dev {count:5d} LWEs -> {d_glwe.numel() * 8} bytes: {fmt(t)}   {info['keyswitches']} automorphism keyswitches, "
              f"{info['launches']} launches, {info['scratch_bytes']} scratch bytes; decrypts: {ok}",
              f"  device-to-host copy of the {d_cts.numel() * 8} bytes of {count} LWEs (pinned): {fmt(copy)}"]
    eng.close()
    ck.close()

    # ---- noise of the host reference against the model ----
    import test_ring_packing as T
    lines.append("noise, host reference on 4,096 packed coefficients of fresh encryptions of 0: measured / modelled variance")
    for p, pr, glwes_n in T.NOISE_CASES:
        lines.append(f"  {p.name} (k = {p.k}, N = {p.N}), pair {pr}: {T.measured_over_modelled(p, pr, glwes_n):.3f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
