#!/usr/bin/env python3
"""Times transciphering on PARAM_MESSAGE_2_CARRY_2 (csrc/transcipher_dev.hip, csrc/transcipher_kernels.hip.h), Kreyvium,
S = 1, 2, 4 strings in lockstep:

  * ms per data round (S x 256 lookups): a next() of 256 characters without the refresh, over its 32 rounds,
  * ks_pbs_dev alone on the same S x 256 rows in the same run, as the comparison,
  * the gather and apply kernels' own times and the ks_pbs level between them (fhe_transcipher_timing: HIP events around
    each phase of every data round),
  * the total for a 256-character string: begin (18 warm-up rounds) + next with the refresh.

HIP events on the stream the engine launches on, after a warm-up run; medians over --reps runs.

    python scripts/transcipher_timing.py [--out profiles/transcipher.txt] [--reps 5]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-string-bounty_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fhestr  # noqa: E402


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcipher.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    cipher, chars = "kreyvium", 256
    bpc, big = fhestr.blocks_per_char(P), P.big_size
    ck = fhestr.ClientKey(P, fhestr.random_seed())
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(*ck.secret_keys(), int.from_bytes(fhestr.random_seed(), "little"))
    stream = torch.cuda.current_stream()
    eng.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    key = rng.bytes(16)
    tc = eng.transcipher(cipher, ck.encrypt_stream_key(cipher, key), max_streams=4)
    med = statistics.median
    lines = [f"transciphering, {P.name}, {cipher}, kernels {fhestr.kernel_revision()}; a {chars}-character string is 18 warm-up rounds of 192 lookups + "
             f"{chars // 8} data rounds of 256 + a refresh of {chars * bpc}, per string",
             f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
             f"HIP events, ms, medians of {args.reps} runs after one warm-up run:"]
    for S in (1, 2, 4):
        ivs = [rng.bytes(16) for _ in range(S)]
        plain = [bytes(rng.integers(0x20, 0x7F, size=chars, dtype=np.uint8)) for _ in range(S)]
        enc = [fhestr.stream_encrypt(cipher, key, iv, s) for iv, s in zip(ivs, plain)]
        d_out = torch.zeros((S, chars * bpc, big), dtype=torch.int64, device="cuda:0")
        rows = S * 256
        d_in = torch.from_numpy(ck.encrypt(np.arange(rows) % 4).view(np.int64)).cuda()
        d_idx = torch.full((rows,), eng.generate_lookup_table(lambda x: x)[0], dtype=torch.int32, device="cuda:0")
        d_pbs = torch.zeros((rows, big), dtype=torch.int64, device="cuda:0")
        t = {"begin": [], "rounds": [], "total": [], "ks_pbs": [], "refresh": []}
        phases = {"gather_ms": [], "ks_pbs_ms": [], "apply_ms": []}
        for rep in range(args.reps + 1):
            begin = timed(stream, lambda: tc.begin(ivs))
            rounds = timed(stream, lambda: tc.next(enc, refresh=False, d_out=d_out.data_ptr()))
            alone = med([timed(stream, lambda: eng.apply_lookup_table_dev(d_in.data_ptr(), d_idx.data_ptr(), d_pbs.data_ptr(), rows)) for _ in range(8)])
            total = timed(stream, lambda: (tc.begin(ivs), tc.next(enc, refresh=True, d_out=d_out.data_ptr())))
            tc.begin(ivs)
            tc.timing(True)
            tc.next(enc, refresh=False, d_out=d_out.data_ptr())
            ph = tc.timing(False)
            if rep == 0:
                continue                                    # the warm-up run
            t["begin"].append(begin); t["rounds"].append(rounds / (chars // 8)); t["total"].append(total); t["ks_pbs"].append(alone)
            for k in phases:
                phases[k].append(ph[k] / ph["rounds"])
        tc.begin(ivs)
        out = tc.next(enc)
        ok = all(fhestr.blocks_to_string(P, ck.decrypt(out[s])) == plain[s].rstrip(b"\0") for s in range(S))
        g, k, a = (med(phases[x]) for x in ("gather_ms", "ks_pbs_ms", "apply_ms"))
        lines += [f"  S = {S} ({rows} lookups per data round); decrypts: {ok}",
                  f"    data round, next() over {chars // 8} rounds   {med(t['rounds']):.3f} ms per round",
                  f"    ks_pbs_dev alone on {rows} rows           {med(t['ks_pbs']):.3f} ms    round / ks_pbs_dev {med(t['rounds']) / med(t['ks_pbs']):.3f}",
                  f"    phases of a data round (timed mode)     gather {g * 1e3:.1f} us, ks_pbs {k:.3f} ms, apply {a * 1e3:.1f} us; "
                  f"gather / ks_pbs_dev alone {g / med(t['ks_pbs']) * 100:.2f} %",
                  f"    warm-up, begin()                         {med(t['begin']):.2f} ms ({med(t['begin']) / 18:.3f} ms per round of {S * 192})",
                  f"    {chars}-character string{'s' if S > 1 else ''}, begin + next with refresh  {med(t['total']):.1f} ms"
                  + (f" ({med(t['total']) / S:.1f} ms per string)" if S > 1 else "")]
    tc.close()
    eng.set_stream(None)
    eng.close()
    ck.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
