"""Single-run times of the slice names (take / skip / split_at / char_at / insert at an encrypted position) beside trim_start's in the
same run, host to host, plan cached: PARAM_MESSAGE_2_CARRY_2 at 32 and 256 characters, device-generated keys, every result decrypted
and compared with Python bytes.  Needs a GPU.  python scripts/slice_timing.py [file to write the table to]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fhe-string-bounty_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import oracle as O
import fhestr
from conftest import to_fhestr_params

P = to_fhestr_params(O.PARAM_MESSAGE_2_CARRY_2_KS_PBS)
ck = fhestr.ClientKey(P, 0x5EED0F00)
eng = fhestr.Engine(P, 0)
eng.generate_keys(*ck.secret_keys(), 0x5EED0F01)
ops = fhestr.FheStringOps(eng)
lines = ["# single run, host to host, plan cached (the second call of each name); MI355X, PARAM_MESSAGE_2_CARRY_2_KS_PBS",
         "# name                      a_cap   n_pbs  levels   ms"]
for cap in (32, 256):
    text = (b"  key:" + bytes(97 + i % 26 for i in range(cap)))[:cap - 3]
    a = np.ascontiguousarray(ck.encrypt(fhestr.string_to_blocks(P, text, cap)))
    t = np.ascontiguousarray(ck.encrypt(fhestr.string_to_blocks(P, b"XY", 4)))
    n = cap // 2 + 1
    count = fhestr.EncryptedCount(np.ascontiguousarray(ck.encrypt(fhestr.encode_count(P, n, cap))), cap)
    calls = [("trim_start", 0, None, lambda: ops.trim_start(a), text.lstrip()),
             (f"take_encn:{cap}", 0, None, lambda: ops.take(a, count), text[:n]),
             (f"skip_encn:{cap}", 0, None, lambda: ops.skip(a, count), text[n:]),
             (f"split_at_encn:{cap}", 0, None, lambda: np.concatenate(ops.split_at(a, count))[:cap * 4], text[:n]),
             (f"char_at_encn:{cap}", 0, None, lambda: ops.char_at(a, count)[1], text[n:n + 1]),
             (f"insert_encn:{cap}", 4, None, lambda: ops.insert(a, count, t), text[:n] + b"XY" + text[n:]),
             (f"insert_encn_clear:{cap}", 0, b"XY", lambda: ops.insert(a, count, b"XY"), text[:n] + b"XY" + text[n:]),
             ("trim_start", 0, None, lambda: ops.trim_start(a), text.lstrip())]
    for name, b_cap, clear, call, want in calls:
        info = fhestr.Plan.string_op(None, name, cap, b_cap, clear, params=P).info()
        call()
        t0 = time.perf_counter()
        out = call()
        ms = (time.perf_counter() - t0) * 1e3
        got = fhestr.blocks_to_string(P, ck.decrypt(np.asarray(out).reshape(-1, P.big_size)))
        lines.append(f"{name:<28}{cap:>5}{info['n_pbs']:>8}{info['n_levels']:>8}{ms:>9.1f}" + ("" if got == want else f"   WRONG {got!r}"))
        print(lines[-1], flush=True)
if len(sys.argv) > 1:                                      # keep the table: python scripts/slice_timing.py profiles/slice.txt
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
ops.close(); eng.close(); ck.close()
