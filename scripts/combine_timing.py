"""Single-run times of the names that combine results (bit logic, select, arithmetic and comparisons on counts) beside trim_start's in
the same run, host to host, plan cached: PARAM_MESSAGE_2_CARRY_2 at 32 characters resp. the bound 32, device-generated keys, every
result decrypted and compared with Python.  Needs a GPU.  python scripts/combine_timing.py [file to write the table to]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fhe-string-bounty_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import oracle as O
import fhestr
from conftest import to_fhestr_params

P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
ck = fhestr.ClientKey(P, 0x5EED0C00)
eng = fhestr.Engine(P, 0)
eng.generate_keys(*ck.secret_keys(), 0x5EED0C01)
ops = fhestr.FheStringOps(eng)
CAP = 32
enc = lambda msgs: np.ascontiguousarray(ck.encrypt(np.asarray(msgs, dtype=np.uint64)))
text, other = b"  key:abcdefghijklmnopqrstuvw", b"the other string"
a, b = enc(fhestr.string_to_blocks(P, text, CAP)), enc(fhestr.string_to_blocks(P, other, CAP))
one, zero = enc([1]), enc([0])
x, y = 21, 13
cx, cy = (fhestr.EncryptedCount(enc(fhestr.encode_count(P, v, CAP)), CAP) for v in (x, y))
string = lambda out: fhestr.blocks_to_string(P, ck.decrypt(np.asarray(out).reshape(-1, P.big_size)))
number = lambda out: fhestr.decode_count(P, ck.decrypt(np.asarray(out.digits if isinstance(out, fhestr.EncryptedCount) else out).reshape(-1, P.big_size)))
PY = {"add": lambda p, q: p + q, "sub": lambda p, q: max(p - q, 0), "eq": lambda p, q: p == q, "ne": lambda p, q: p != q,
      "lt": lambda p, q: p < q, "le": lambda p, q: p <= q, "gt": lambda p, q: p > q, "ge": lambda p, q: p >= q}
# (plan name, a_cap, b_cap, clear, the call, how its result decodes, what Python says)
calls = [("trim_start", CAP, 0, None, lambda: ops.trim_start(a), string, text.lstrip()),
         ("and:2", 0, 0, None, lambda: ops.bit_and(one, zero), number, 0), ("or:2", 0, 0, None, lambda: ops.bit_or(one, zero), number, 1),
         ("xor:2", 0, 0, None, lambda: ops.bit_xor(one, one), number, 0), ("not:1", 0, 0, None, lambda: ops.bit_not(zero), number, 1),
         (f"select:{CAP}", CAP, CAP, None, lambda: ops.select(zero, a, b), string, other),
         (f"select_clear:{CAP}", CAP, 0, other, lambda: ops.select(one, a, other), string, text),
         (f"select_count:{CAP}:{CAP}", 0, 0, None, lambda: ops.select(one, cx, cy), number, x)]
for op in PY:
    calls.append((f"count_{op}:{CAP}:{CAP}", 0, 0, None, lambda op=op: getattr(ops, f"count_{op}")(cx, cy), number, int(PY[op](x, y))))
for op in PY:
    calls.append((f"count_{op}_clear:{CAP}", 0, 0, b"\x01", lambda op=op: getattr(ops, f"count_{op}")(cx, 1), number, int(PY[op](x, 1))))
calls.append(calls[0])
lines = ["# single run, host to host, plan cached (the second call of each name); MI355X, PARAM_MESSAGE_2_CARRY_2_KS_PBS, 32 characters / bound 32",
         "# name                       n_pbs  levels   ms"]
for name, a_cap, b_cap, clear, call, decode, want in calls:
    info = fhestr.Plan.string_op(None, name, a_cap, b_cap, clear, params=P).info()
    call()
    t0 = time.perf_counter()
    out = call()
    ms = (time.perf_counter() - t0) * 1e3
    got = decode(out)
    lines.append(f"{name:<28}{info['n_pbs']:>6}{info['n_levels']:>8}{ms:>9.1f}" + ("" if got == want else f"   WRONG {got!r}"))
    print(lines[-1], flush=True)
if len(sys.argv) > 1:                                      # keep the table: python scripts/combine_timing.py profiles/combine.txt
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
ops.close(); eng.close(); ck.close()
