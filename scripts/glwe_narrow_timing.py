#!/usr/bin/env python3
"""Times the narrow packed results on PARAM_MESSAGE_2_CARRY_2 (csrc/glwe_narrow_kernels.hip.h), 1,024 rows:

  * narrow_sample_extract_kernel (Engine.unpack_narrow, refresh=False) next to glwe_sample_extract_kernel (Engine.unpack)
    on the same rows, at b = 13, 16 and 32: both write the same 16.8 MB,
  * glwe_narrow_kernel alone (Engine.narrow on device buffers),
  * the two-step alternative: glwe_widen_kernel to full GLWEs in HBM, then glwe_sample_extract_kernel,
  * the PCIe bytes of the chained example contains(to_upper(hay, packed=Narrow()), pat) against packed=True.

HIP events on the stream the engine launches on, after warm-up; medians over --reps launches, --rounds interleaved rounds.

    python scripts/glwe_narrow_timing.py [--out profiles/glwe_narrow.txt] [--reps 50] [--rounds 5]"""
import argparse
import os
import statistics
import sys

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
        ms.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glwe_narrow.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    rows, big = 1024, P.big_size
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), int.from_bytes(fhestr.random_seed(), "little"))
    pp = (7, 3)                                             # the pair under which a width is operand-grade on this set
    eng.load_packing_key(*ck.gen_packing_key(pp, seed=fhestr.random_seed()))
    stream = torch.cuda.current_stream()
    eng.set_stream(stream.cuda_stream)

    M = P.msg_mod * P.carry_mod
    msgs = np.arange(rows) % M
    d_glwe = torch.from_numpy(eng.pack(ck.encrypt(msgs)).view(np.int64)).cuda()
    d_wide = torch.zeros_like(d_glwe)
    d_out = torch.zeros((rows, big), dtype=torch.int64).cuda()
    mb = rows * big * 8 / 1e6
    lines = [f"narrow packed results, {P.name}, kernels {fhestr.kernel_revision()}, packing pair {pp}: operand-grade width "
             f"{fhestr.narrow_default_bits(P, pp, True)} bits, client-grade {fhestr.narrow_default_bits(P, pp, False)} bits",
             f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"HIP events, us, medians of {args.reps} launches after 5 warm-up launches, {args.rounds} interleaved rounds; {rows} rows, "
             f"{mb:.1f} MB written by every extraction:"]
    full = lambda src=d_glwe: eng.unpack(d_in=src.data_ptr(), count=rows, refresh=False, d_out=d_out.data_ptr())
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)
    for b in (13, 16, 32):
        d_narrow = torch.zeros((fhestr.narrow_len(P, rows, b),), dtype=torch.int64).cuda()
        narrow = lambda: eng.narrow(d_in=d_glwe.data_ptr(), held=rows, bits=b, d_out=d_narrow.data_ptr())
        fused = lambda: eng.unpack_narrow(d_in=d_narrow.data_ptr(), held=rows, bits=b, refresh=False, d_out=d_out.data_ptr())
        widen = lambda: eng.widen(d_narrow.data_ptr(), rows, b, d_wide.data_ptr())
        two_step = lambda: (widen(), full(d_wide))
        narrow()
        t = {"full": [], "fused": [], "two": [], "narrow": [], "widen": []}
        for _ in range(args.rounds):
            t["full"].append(timed(stream, full, args.reps))
            t["fused"].append(timed(stream, fused, args.reps))
            t["two"].append(timed(stream, two_step, args.reps))
            t["narrow"].append(timed(stream, narrow, args.reps))
            t["widen"].append(timed(stream, widen, args.reps))
        fused()
        stream.synchronize()
        a = d_out.cpu().numpy().view(np.uint64).copy()
        two_step()
        stream.synchronize()
        same = np.array_equal(a, d_out.cpu().numpy().view(np.uint64))
        ok = np.array_equal(ck.decrypt(a), msgs)
        m = {k: statistics.median(v) for k, v in t.items()}
        lines += [f"  b = {b}: the list is {d_narrow.numel() * 8} bytes against {d_glwe.numel() * 8}",
                  f"    glwe_sample_extract_kernel (full GLWEs)  round medians {fmt(t['full'])} -> {m['full']:.1f} us = {mb / m['full']:.2f} TB/s written",
                  f"    narrow_sample_extract_kernel (fused)     round medians {fmt(t['fused'])} -> {m['fused']:.1f} us = {mb / m['fused']:.2f} TB/s written; "
                  f"fused / full {m['fused'] / m['full']:.3f}; decrypts: {ok}",
                  f"    two steps: glwe_widen_kernel + glwe_sample_extract_kernel  round medians {fmt(t['two'])} -> {m['two']:.1f} us; "
                  f"fused / two steps {m['fused'] / m['two']:.3f}; same words as fused: {same}",
                  f"    glwe_widen_kernel alone  round medians {fmt(t['widen'])} -> {m['widen']:.1f} us",
                  f"    glwe_narrow_kernel alone round medians {fmt(t['narrow'])} -> {m['narrow']:.1f} us"]
    eng.set_stream(None)
    ops = fhestr.FheStringOps(eng)
    cap, pcap = 32, 8
    n, np_ = cap * ops.bpc, pcap * ops.bpc
    lwe, glwe = big * 8, (P.k + 1) * P.N * 8
    hay = ck.encrypt(fhestr.string_to_blocks(P, b"the quick brown fox", cap))
    pat = ck.encrypt(fhestr.string_to_blocks(P, b"BROWN", pcap))
    up = ops.to_upper(hay, packed=fhestr.Narrow())
    got = ck.decrypt(ops.contains(up, pat).reshape(1, -1))[0]
    nb = up.nbytes
    lines += [f"  chained contains(to_upper(hay), pat), hay {cap} chars = {n} blocks, pat {pcap} chars = {np_} blocks, result {got}; bytes over PCIe:",
              f"    packed=True:     up {n * lwe} + down {glwe} (to_upper), up {glwe} + {np_ * lwe} + down {lwe} (contains) = {(n + np_ + 1) * lwe + 2 * glwe}; "
              f"the stored string: {glwe} bytes",
              f"    packed=Narrow(): up {n * lwe} + down {nb} (to_upper, {up.bits} bits), up {nb} + {np_ * lwe} + down {lwe} (contains) = "
              f"{(n + np_ + 1) * lwe + 2 * nb}; the stored string: {nb} bytes"]
    ops.close()
    eng.close()
    ck.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
