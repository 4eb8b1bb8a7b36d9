"""Compact public-key ciphertext lists: what the device expansion costs and what it saves (GPU box; output kept in
profiles/compact_expand.txt).

  python scripts/compact_bench.py [--out FILE]      runs the three sections below, each in a process of its own under
                                                    `timeout`; the first one that fails ends the run
  --section kernel   compact_expand_kernel against a hipMemcpyAsync device-to-device copy of exactly the output's bytes
                     (HIP events, warm, median of 20, five alternating repetitions): PARAM_MESSAGE_2_CARRY_2 at 1,024 and
                     32,768 rows, PARAM_MESSAGE_4_CARRY_4 at 2,048 rows.  The copy is the memory system's own rate for
                     "write this many bytes"; the expansion writes the same bytes and reads 1/n of them.  Held against:
                     kernel median <= copy median + the copy's own spread (max - min of its five medians).  Below about
                     20 us both are launch-bound: reported, not judged.
  --section route    to_lower on a 1,024-char string and eq on 32 strings of 256 chars (PARAM_MESSAGE_2_CARRY_2), wall
                     time from before the upload to the completion of the operation, median of 10 alternating pairs:
                     (a) inputs uploaded as expanded ciphertexts from pinned host memory, (b) uploaded as a compact list
                     and expanded on the device.  Held against: (b) not slower than (a) in any pair.
  --section client   host milliseconds to make a public key and to encrypt one full bin, P22 and P44, 1 and 16 threads.
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-string-bounty_amd"))

SECTIONS = (("client", 300), ("kernel", 240), ("route", 420))


def drive(out_path):
    lines = []
    for name, limit in SECTIONS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--section", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            lines.append(f"section {name} ended with status {r.returncode}: stopping here\n")
            sys.stdout.write(lines[-1])
            break
    if out_path:
        with open(out_path, "w") as fh:
            fh.writelines(lines)
    return r.returncode


class Hip:
    """The few runtime calls the measurements need, from the runtime the engine already lives in."""

    def __init__(self):
        import fhestr
        fhestr.lib()
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                self.L = C.CDLL(name)
                break
            except OSError:
                continue
        else:
            raise RuntimeError("libamdhip64 not found")
        vp = C.c_void_p
        self.L.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
        self.L.hipFree.argtypes = [vp]
        self.L.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        self.L.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
        self.L.hipEventCreate.argtypes = [C.POINTER(vp)]
        self.L.hipEventRecord.argtypes = [vp, vp]
        self.L.hipEventSynchronize.argtypes = [vp]
        self.L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        self.L.hipStreamSynchronize.argtypes = [vp]

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP call failed with status {rc}")

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), nbytes))
        return p.value

    def free(self, p):
        self.ok(self.L.hipFree(C.c_void_p(p)))

    def copy(self, dst, src, nbytes, kind, stream):      # kind: 1 host to device, 2 device to host, 3 device to device
        self.ok(self.L.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, kind, C.c_void_p(stream)))

    def event(self):
        e = C.c_void_p()
        self.ok(self.L.hipEventCreate(C.byref(e)))
        return e

    def timed(self, stream, launch, reps=20):
        """HIP-event time of every one of `reps` launches on `stream`, microseconds."""
        pairs = [(self.event(), self.event()) for _ in range(reps)]
        for a, b in pairs:
            self.ok(self.L.hipEventRecord(a, C.c_void_p(stream)))
            launch()
            self.ok(self.L.hipEventRecord(b, C.c_void_p(stream)))
        self.ok(self.L.hipStreamSynchronize(C.c_void_p(stream)))
        out = []
        for a, b in pairs:
            ms = C.c_float()
            self.ok(self.L.hipEventElapsedTime(C.byref(ms), a, b))
            out.append(ms.value * 1e3)
        return out


def section_kernel():
    import numpy as np
    import fhestr
    hip = Hip()
    print("== kernel: compact_expand_kernel against a device-to-device copy of the output's bytes (HIP events, us) ==")
    for P, rows in ((fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 1024), (fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS, 32768),
                    (fhestr.PARAM_MESSAGE_4_CARRY_4_KS_PBS, 2048)):
        eng = fhestr.Engine(P, 0)
        stream = eng.stream
        nbytes = rows * P.big_size * 8
        clist = np.random.default_rng(rows).integers(0, 2**64, size=fhestr.compact_list_len(P, rows), dtype=np.uint64)
        d_list, d_out, d_src, d_dst = hip.malloc(clist.nbytes), hip.malloc(nbytes), hip.malloc(nbytes), hip.malloc(nbytes)
        hip.copy(d_list, clist.ctypes.data, clist.nbytes, 1, stream)
        hip.ok(hip.L.hipMemsetAsync(C.c_void_p(d_src), 0x5A, nbytes, C.c_void_p(stream)))
        eng.synchronize()
        expand = lambda: eng.expand_compact_list(None, rows, d_out=d_out, d_list=d_list)
        copy = lambda: hip.copy(d_dst, d_src, nbytes, 3, stream)
        hip.timed(stream, expand, 5), hip.timed(stream, copy, 5)            # warm
        k_med, c_med = [], []
        for _ in range(5):
            k_med.append(statistics.median(hip.timed(stream, expand)))
            c_med.append(statistics.median(hip.timed(stream, copy)))
        # the result that was timed is the right one
        got = np.empty(rows * P.big_size, dtype=np.uint64)
        hip.copy(got.ctypes.data, d_out, nbytes, 2, stream)
        eng.synchronize()
        assert np.array_equal(got.reshape(rows, P.big_size), fhestr.expand_compact_host(P, clist, rows))
        k, c, spread = statistics.median(k_med), statistics.median(c_med), max(c_med) - min(c_med)
        if max(k, c) < 20:
            verdict = "launch-bound, not judged"
        elif k <= c + spread:
            verdict = "within the copy's time"
        else:
            verdict = f"OVER the copy's time plus its spread by {k - c - spread:.1f} us"
        print(f"{P.name} rows {rows:6d}  {nbytes / 1e6:8.1f} MB out, {clist.nbytes / 1e3:8.1f} KB in | expand medians "
              f"{' '.join(f'{v:.1f}' for v in k_med)} -> {k:.1f} us = {nbytes / k / 1e6:.2f} TB/s written | copy medians "
              f"{' '.join(f'{v:.1f}' for v in c_med)} -> {c:.1f} us = {nbytes / c / 1e6:.2f} TB/s copied, spread {spread:.1f} | {verdict}")
        for p in (d_list, d_out, d_src, d_dst):
            hip.free(p)
        eng.close()


def section_route():
    import numpy as np
    import fhestr
    hip = Hip()
    P = fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS
    big, bpc = P.big_size, fhestr.blocks_per_char(P)
    ck = fhestr.ClientKey(P, 0xBE7C4)
    pk = ck.compact_public_key(0xBE7C5)
    g, s = ck.secret_keys()
    eng = fhestr.Engine(P, 0)
    eng.generate_keys(g, s, 0xBE7C6)
    stream = eng.stream
    rng = np.random.default_rng(3)
    print("== route: wall ms from before the upload to the completion of the operation, outputs resident ==")

    def pinned(a):
        buf = fhestr.pinned_empty(a.shape)
        buf[...] = a
        return buf

    def pairs(route_a, route_b, reps=10):
        route_a(), route_b()                                             # warm: plans, staging buffers, code objects
        ta, tb = [], []
        for _ in range(reps):
            for route, acc in ((route_a, ta), (route_b, tb)):
                eng.synchronize()
                t0 = time.perf_counter()
                route()
                acc.append((time.perf_counter() - t0) * 1e3)
        return ta, tb

    def report(name, ta, tb, bytes_a, bytes_b):
        slower = sum(1 for x, y in zip(ta, tb) if y > x)
        print(f"{name}: (a) expanded upload {bytes_a / 1e6:.1f} MB over PCIe, median {statistics.median(ta):.2f} ms "
              f"[{min(ta):.2f} .. {max(ta):.2f}] | (b) compact list {bytes_b / 1e3:.1f} KB over PCIe + device expansion, median "
              f"{statistics.median(tb):.2f} ms [{min(tb):.2f} .. {max(tb):.2f}] | (b) - (a) = "
              f"{statistics.median(tb) - statistics.median(ta):+.2f} ms | (b) slower than (a) in {slower} of {len(ta)} pairs")
        print("  pairs (a, b): " + " ".join(f"({x:.2f}, {y:.2f})" for x, y in zip(ta, tb)))

    # to_lower on one 1,024-char string
    text = bytes(rng.integers(0x41, 0x7B, size=1000, dtype=np.uint8))
    count = 1024 * bpc
    clist = pinned(pk.encrypt_string(text, 1024, 1))
    expanded = pinned(fhestr.expand_compact_host(P, clist, count))
    plan = fhestr.Plan.string_op(eng, "to_lower", 1024)
    n_out = plan.info()["n_outputs"]
    d_in, d_res = hip.malloc(count * big * 8), hip.malloc(n_out * big * 8)

    def lower_a():
        hip.copy(d_in, expanded.ctypes.data, expanded.nbytes, 1, stream)
        plan.run_dev(d_in, d_res)
        eng.synchronize()

    def lower_b():
        eng.expand_compact_list(clist, count, d_out=d_in)
        plan.run_dev(d_in, d_res)
        eng.synchronize()

    ta, tb = pairs(lower_a, lower_b)
    res = np.empty((n_out, big), dtype=np.uint64)
    hip.copy(res.ctypes.data, d_res, res.nbytes, 2, stream)
    eng.synchronize()
    assert fhestr.blocks_to_string(P, ck.decrypt(res)) == text.lower()
    report("to_lower, 1,024 chars", ta, tb, expanded.nbytes, clist.nbytes)
    hip.free(d_in), hip.free(d_res)
    plan.close()
    del expanded

    # eq of 32 strings of 256 chars against one pattern (the fhe_str_op_many shape)
    rows_txt = [bytes(rng.integers(0x61, 0x7B, size=256, dtype=np.uint8)) for _ in range(32)]
    pat = rows_txt[5]
    per = 256 * bpc
    # (a): the parent's route, fhe_str_op_many from pinned host memory (32 rows + the pattern once; the 32 result
    # ciphertexts come back to the host, 0.5 MB)
    rows_list = pk.encrypt(np.concatenate([fhestr.string_to_blocks(P, t, 256) for t in rows_txt]), 2)
    rows = pinned(fhestr.expand_compact_host(P, rows_list, 32 * per).reshape(32, per, big))
    b = pinned(fhestr.expand_compact_host(P, pk.encrypt_string(pat, 256, 3), per))
    out_buf = fhestr.pinned_empty((32, 1, big))
    ops = fhestr.FheStringOps(eng, out_alloc=lambda shape: out_buf)
    # (b): every instance's (row, pattern) pair in one compact list, expanded into the layout fhe_plan_run_batch_dev reads
    both = pinned(pk.encrypt(np.concatenate([np.concatenate([fhestr.string_to_blocks(P, t, 256), fhestr.string_to_blocks(P, pat, 256)])
                                             for t in rows_txt]), 4))
    plan = fhestr.Plan.string_op(eng, "eq", 256, 256)
    d_in, d_res = hip.malloc(32 * 2 * per * big * 8), hip.malloc(32 * big * 8)

    def eq_a():
        ops.op_many("eq", rows, b)

    def eq_b():
        eng.expand_compact_list(both, 32 * 2 * per, d_out=d_in)
        plan.run_batch_dev(d_in, d_res, 32)
        eng.synchronize()

    ta, tb = pairs(eq_a, eq_b)
    res = np.empty((32, big), dtype=np.uint64)
    hip.copy(res.ctypes.data, d_res, res.nbytes, 2, stream)
    eng.synchronize()
    want = [int(t == pat) for t in rows_txt]
    assert list(ck.decrypt(res)) == want and list(ck.decrypt(out_buf[:, 0])) == want
    report("eq, 32 x 256 chars", ta, tb, rows.nbytes + b.nbytes, both.nbytes)
    print("  (b) writes the pattern once per row: 32 x 2,048 ciphertexts = 1.07 GB expanded in HBM against 554 MB uploaded by (a)")
    hip.free(d_in), hip.free(d_res)
    plan.close()                                                         # plans go before their engine
    del ops
    eng.close()


def section_client():
    import numpy as np
    import fhestr
    print("== client: host ms (no GPU involved) ==")
    for P in (fhestr.PARAM_MESSAGE_2_CARRY_2_KS_PBS, fhestr.PARAM_MESSAGE_4_CARRY_4_KS_PBS):
        n = P.k * P.N
        ck = fhestr.ClientKey(P, 1)
        t0 = time.perf_counter()
        pk = ck.compact_public_key(2)
        t_pk = (time.perf_counter() - t0) * 1e3
        msgs = np.arange(n, dtype=np.uint64) % P.msg_mod
        t_enc = {}
        for threads in (1, 16):
            t0 = time.perf_counter()
            clist = pk.encrypt(msgs, 3, threads=threads)
            t_enc[threads] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(ck.decrypt(fhestr.expand_compact_host(P, clist, n)[:64]), msgs[:64].astype(np.int64))
        print(f"{P.name} (n = {n}): public key {t_pk:.1f} ms (up to 16 threads); one full bin of {n} ciphertexts "
              f"{t_enc[1]:.1f} ms on 1 thread, {t_enc[16]:.1f} ms on 16; list {clist.nbytes / 1e3:.1f} KB against "
              f"{n * P.big_size * 8 / 1e6:.1f} MB expanded")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=[s for s, _ in SECTIONS])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.section:
        {"kernel": section_kernel, "route": section_route, "client": section_client}[a.section]()
    else:
        sys.exit(drive(a.out))
