#!/usr/bin/env python3
"""Times the sample extraction of packed inputs on PARAM_MESSAGE_2_CARRY_2 (csrc/glwe_extract_kernels.hip.h):

  * Engine.unpack(refresh=False) on device buffers for 1,024 rows (16.8 MB written) next to compact_expand_kernel on the same
    row count in the same process (the same bytes per row, the same store shape), interleaved rounds,
  * the refresh of 1,024 blocks (extraction + one keyswitch + PBS with the identity table) next to one 1,024-LWE
    apply_lookup_table_dev call,
  * the PCIe bytes of the chained example contains(to_upper(hay, packed=True), pat), expanded against packed.

HIP events on the stream the engine launches on, after warm-up; medians over --reps launches, --rounds rounds.

    python scripts/glwe_extract_timing.py [--out profiles/glwe_extract.txt] [--reps 50] [--rounds 5]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glwe_extract.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    rows, big = 1024, P.big_size
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), int.from_bytes(fhestr.random_seed(), "little"))
    pp = (7, 3)                                             # the default (7, 2) is refused for the refresh on this set
    eng.load_packing_key(*ck.gen_packing_key(pp, seed=fhestr.random_seed()))
    stream = torch.cuda.current_stream()
    eng.set_stream(stream.cuda_stream)

    M = P.msg_mod * P.carry_mod
    msgs = np.arange(rows) % M
    d_glwe = torch.from_numpy(eng.pack(ck.encrypt(msgs)).view(np.int64)).cuda()
    rng = np.random.default_rng(1)
    d_list = torch.from_numpy(rng.integers(0, 2**63, size=fhestr.compact_list_len(P, rows), dtype=np.int64)).cuda()
    d_out = torch.zeros((rows, big), dtype=torch.int64).cuda()
    extract = lambda: eng.unpack(d_in=d_glwe.data_ptr(), count=rows, refresh=False, d_out=d_out.data_ptr())
    expand = lambda: eng.expand_compact_list(None, rows, d_out=d_out.data_ptr(), d_list=d_list.data_ptr())
    ex, cp = [], []
    for _ in range(args.rounds):
        ex.append(timed(stream, extract, args.reps))
        cp.append(timed(stream, expand, args.reps))
    extract()
    stream.synchronize()
    ok = np.array_equal(ck.decrypt(d_out.cpu().numpy().view(np.uint64)), msgs)
    mb = rows * big * 8 / 1e6
    e, c = statistics.median(ex), statistics.median(cp)
    lines = [f"sample extraction of packed inputs, {P.name}, kernels {fhestr.kernel_revision()}",
             f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"HIP events, us, medians of {args.reps} launches after 5 warm-up launches, {args.rounds} interleaved rounds:",
             f"  glwe_sample_extract_kernel {rows} rows, {mb:.1f} MB written, {d_glwe.numel() * 8} bytes read: round medians "
             f"{' '.join(f'{v:.1f}' for v in ex)} -> {e:.1f} us = {mb / e:.2f} TB/s written; decrypts: {ok}",
             f"  compact_expand_kernel      {rows} rows, {mb:.1f} MB written, {d_list.numel() * 8} bytes read: round medians "
             f"{' '.join(f'{v:.1f}' for v in cp)} -> {c:.1f} us = {mb / c:.2f} TB/s written",
             f"  extraction / expansion per byte written: {e / c:.3f} (spread of the rounds: extraction {max(ex) - min(ex):.1f} us, "
             f"expansion {max(cp) - min(cp):.1f} us)"]
    lut_id, _ = eng.generate_lookup_table(lambda x: x)
    d_idx = torch.full((rows,), lut_id, dtype=torch.int32).cuda()
    d_in = torch.from_numpy(ck.encrypt(msgs).view(np.int64)).cuda()
    refresh = timed(stream, lambda: eng.unpack(d_in=d_glwe.data_ptr(), count=rows, refresh=True, d_out=d_out.data_ptr()), 20)
    stream.synchronize()
    ok = np.array_equal(ck.decrypt(d_out.cpu().numpy().view(np.uint64)), msgs)
    pbs = timed(stream, lambda: eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), rows), 20)
    raw, budget = fhestr.packing_unpack_noise(P, pp)
    lines += [f"  unpack with refresh, {rows} blocks (extraction + memset of the indices + ks_pbs, packing pair {pp}: raw block {raw:.2f} "
              f"nominal variances, budget {budget:.0f}): {refresh:.1f} us; decrypts: {ok}",
              f"  one {rows}-LWE apply_lookup_table_dev call on resident ciphertexts: {pbs:.1f} us"]
    eng.set_stream(None)
    ops = fhestr.FheStringOps(eng)
    cap, pcap = 32, 8
    n, np_ = cap * ops.bpc, pcap * ops.bpc
    lwe, glwe = big * 8, (P.k + 1) * P.N * 8
    hay = ck.encrypt(fhestr.string_to_blocks(P, b"the quick brown fox", cap))
    pat = ck.encrypt(fhestr.string_to_blocks(P, b"BROWN", pcap))
    got = ck.decrypt(ops.contains(ops.to_upper(hay, packed=True), pat).reshape(1, -1))[0]
    lines += [f"  chained contains(to_upper(hay), pat), hay {cap} chars = {n} blocks, pat {pcap} chars = {np_} blocks, result {got}; bytes over PCIe:",
              f"    expanded: up {n * lwe} + down {n * lwe} (to_upper), up {(n + np_) * lwe} + down {lwe} (contains) = {(3 * n + np_ + 1) * lwe}",
              f"    packed:   up {n * lwe} + down {glwe} (to_upper, packed=True), up {glwe} + {np_ * lwe} + down {lwe} (contains) = "
              f"{(n + np_ + 1) * lwe + 2 * glwe}; the stored string: {glwe} bytes against {n * lwe}"]
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
