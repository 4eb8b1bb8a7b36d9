#!/usr/bin/env python3
"""Times the packing keyswitch on PARAM_MESSAGE_2_CARRY_2 (csrc/packing_ks_kernels.hip.h) and what it replaces:

  * Engine.pack on device buffers (fhe_engine_pack_lwes_dev: memset + digits + product with the rotate-and-sum epilogue)
    for 256 and for 1024 LWEs,
  * the device-to-host copy of the 1024 x 2049 words (16.8 MB) a 256-character result occupies as LWEs, into pinned memory,
  * a 256-character to_lower from the same run (host arrays in, host arrays out), and the same with packed=True,
  * the bytes the packing key occupies in HBM, from the kernel's geometry.

HIP events on the stream the engine launches on, after warm-up; medians over --reps launches.  Writes a text report.

    python scripts/packing_ks_timing.py [--out profiles/packing_ks.txt] [--reps 50]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-string-bounty_amd"))

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packing_ks.txt"))
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    eng = fhestr.Engine(P, 0)
    glwe_sk, small_sk = ck.secret_keys()
    eng.generate_keys(glwe_sk, small_sk, int.from_bytes(fhestr.random_seed(), "little"))
    t0 = time.perf_counter()
    pp, key = ck.gen_packing_key(seed=fhestr.random_seed())
    keygen_s = time.perf_counter() - t0
    eng.load_packing_key(pp, key)
    stream = torch.cuda.current_stream()
    eng.set_stream(stream.cuda_stream)

    epg = 16 // pp[1]
    steps, col_groups = -(-P.k * P.N // (2 * epg)), (P.k + 1) * P.N // 32
    plane_bytes = col_groups * steps * 8 * 1024
    lines = [f"packing keyswitch, {P.name}, decomposition base_log {pp[0]} x {pp[1]} levels, kernels {fhestr.kernel_revision()}",
             f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"key: {key.nbytes} bytes as 64-bit words on the wire; {plane_bytes} bytes in HBM as int8 digit planes "
             f"({col_groups} column groups x {steps} K steps x 8 planes x 1024 bytes, {epg} mask elements per 16-slot group); "
             f"CPU generation {keygen_s:.2f} s",
             f"HIP events, median (min .. max) of {args.reps} launches after 5 warm-up launches:"]
    msgs = np.arange(1024) % (P.msg_mod * P.carry_mod)
    d_cts = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    d_glwe = torch.zeros((1, P.k + 1, P.N), dtype=torch.int64).cuda()
    for count in (256, 1024):
        med, lo, hi = timed(stream, lambda: eng.pack(d_in=d_cts.data_ptr(), count=count, d_out=d_glwe.data_ptr()), args.reps)
        info = eng.packing_info()
        stream.synchronize()
        ok = np.array_equal(ck.decrypt_packed(d_glwe.cpu().numpy().view(np.uint64), count), msgs[:count])
        lines.append(f"  pack_lwes_dev {count:5d} LWEs -> {d_glwe.numel() * 8} bytes: {med * 1e3:8.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})   "
                     f"tile {info['tile']}, {info['chunks']} K chunks of {info['steps_per_chunk']} of {info['steps']} steps; decrypts: {ok}")
    host = torch.empty(d_cts.shape, dtype=torch.int64).pin_memory()
    med, lo, hi = timed(stream, lambda: host.copy_(d_cts, non_blocking=True), args.reps)
    lines.append(f"  device-to-host copy of the {d_cts.numel() * 8} bytes of 1024 LWEs (pinned): {med * 1e3:8.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    host_small = torch.empty(d_glwe.shape, dtype=torch.int64).pin_memory()
    med, lo, hi = timed(stream, lambda: host_small.copy_(d_glwe, non_blocking=True), args.reps)
    lines.append(f"  device-to-host copy of the {d_glwe.numel() * 8} bytes of one GLWE (pinned):      {med * 1e3:8.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")

    eng.set_stream(None)
    ops = fhestr.FheStringOps(eng, out_alloc=fhestr.pinned_empty)
    s = (b"The Quick Brown Fox Jumps Over The Lazy Dog. " * 6)[:256]
    es = ck.encrypt(fhestr.string_to_blocks(P, s, 256))
    ops.to_lower(es)
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = ops.to_lower(es)
        wall.append((time.perf_counter() - t0) * 1e3)
    ok = fhestr.blocks_to_string(P, ck.decrypt(out)) == s.lower()
    lines.append(f"  256-character to_lower, host arrays in and out (wall clock, median of 5): {statistics.median(wall):.2f} ms; decrypts: {ok}")
    ops.to_lower(es, packed=True)                           # builds and keeps the plan
    t0 = time.perf_counter()
    packed = ops.to_lower(es, packed=True)
    wall_packed = (time.perf_counter() - t0) * 1e3
    ok = fhestr.blocks_to_string(P, ck.decrypt_packed(packed, 1024)) == s.lower()
    lines.append(f"  the same with packed=True (plan on device buffers, packed there, 32 KB downloaded; second run): {wall_packed:.2f} ms; decrypts: {ok}")
    eng.close()
    ck.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
