"""Randomised differential test of every FheString operation against Python bytes semantics on the GPU
(toy parameters: a PBS costs ~0.1 ms).  Usage: python scripts/fuzz_strings.py [cases] [seed]
FUZZ_PARAMS=n32768 runs it on 4-bit blocks (msg_mod = carry_mod = 16 on N = 32768, toy n): the whole-character and
pattern-class circuits of PARAM_MESSAGE_4_CARRY_4."""
import os
import sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "fhe-string-bounty_amd")
sys.path.insert(0, "tests")
import oracle as O
import fhestr
from split_ref import ONCE, SPLIT_OPS, decode_split, split_ref        # the clear-text definitions of the split family
from count_ref import repeat_ref, replacen_ref, splitn_ref            # ... and of the operations with an encrypted count
from slice_ref import decode_slice, slice_ref                         # ... and of the slices at a clear or an encrypted position
from combine_ref import COUNT_OPS, bits_ref, count_bound, count_ref, decode_bit, decode_digits, decode_string, select_ref   # ... and of what combines results

N_CASES = int(sys.argv[1]) if len(sys.argv) > 1 else 150
SEED = int(sys.argv[2]) if len(sys.argv) > 2 else 1
p = O.TOY_N32768 if os.environ.get("FUZZ_PARAMS") == "n32768" else O.TOY_K1
ck = O.ClientKey(p, 0xF022)
sk = O.ServerKey(ck, fourier=False)
P = fhestr.Params(p.n, p.k, p.N, p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.msg_mod, p.carry_mod,
                  p.lwe_std, p.glwe_std, p.name)
eng = fhestr.Engine(P, 0)
eng.load_keys(sk.bsk, sk.ksk)
ops = fhestr.FheStringOps(eng)
rng = np.random.default_rng(SEED)
enc = lambda s, cap: ck.encrypt_many(fhestr.string_to_blocks(P, s, cap))
dec = lambda ct: ck.decrypt_many(np.asarray(ct).reshape(-1, p.big_size))
dec_str = lambda ct: fhestr.blocks_to_string(P, dec(ct))
ALPHA = b"abAB \t\nxyz.Zq"
WS = b" \t\n\x0b\x0c\r"


def rand_str(max_len):
    n = int(rng.integers(0, max_len + 1))
    return bytes(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), size=n))


def digits_to_int(d):
    return sum(int(v) * (p.msg_mod ** i) for i, v in enumerate(d))


fails = slices = combines = 0
def check(name, got, want, ctx):
    global fails
    if got != want:
        fails += 1
        print(f"MISMATCH {name}: got {got!r} want {want!r} ctx {ctx!r}", flush=True)


for case in range(N_CASES):
    # 20 / 24: more than msg*carry = 16 candidate offsets, so reductions and prefix scans meet runs of exactly 16 bits
    cap = int(rng.choice([2, 3, 4, 6, 8, 20] if p.msg_mod == 4 else [3, 4, 6, 8, 12, 24]))
    a = rand_str(cap)
    # patterns: often substrings of a so that positive cases are frequent
    if len(a) and rng.random() < 0.6:
        i = int(rng.integers(0, len(a))); j = int(rng.integers(i, len(a) + 1))
        b = a[i:j]
    else:
        b = rand_str(min(cap, 4))
    b_cap = max(1, int(rng.choice([len(b), min(cap, max(len(b), 1) + 1)])))
    if b_cap < len(b): b_cap = len(b)
    ea, eb = enc(a, cap), enc(b, b_cap)
    op = str(rng.choice(["eq", "ne", "lt", "le", "gt", "ge", "eqic", "starts", "ends", "contains", "find", "rfind",
                         "upper", "lower", "trim_start", "trim_end", "strip", "replace", "len", "is_empty",
                         "strip_prefix", "strip_suffix", "concat", "repeat", "replace_general", "split", "split_ws", "replacen",
                         "repeat_encn", "replacen_encn", "splitn_encn", "rsplitn_encn", "slice", "slice", "combine", "combine"]))
    clear = bool(rng.random() < 0.5)
    rhs = b if clear else eb
    ctx = (op, a, b, cap, b_cap, clear)
    if op in ("eq", "ne", "lt", "le", "gt", "ge"):
        if not clear and b_cap != cap:      # compare equal capacities or clear
            eb2 = enc(b[:cap], cap); b2 = b[:cap]; rhs = eb2
        else:
            b2 = b
        want = {"eq": a == b2, "ne": a != b2, "lt": a < b2, "le": a <= b2, "gt": a > b2, "ge": a >= b2}[op]
        check(op, int(dec(getattr(ops, op)(ea, rhs))[0]), int(want), ctx)
    elif op == "eqic":
        check(op, int(dec(ops.eq_ignore_case(ea, rhs))[0]), int(a.lower() == b.lower()), ctx)
    elif op == "starts":
        check(op, int(dec(ops.starts_with(ea, rhs))[0]), int(a.startswith(b)), ctx)
    elif op == "ends":
        check(op, int(dec(ops.ends_with(ea, rhs))[0]), int(a.endswith(b)), ctx)
    elif op == "contains":
        check(op, int(dec(ops.contains(ea, rhs))[0]), int(b in a), ctx)
    elif op in ("find", "rfind"):
        r = dec(getattr(ops, op)(ea, rhs))
        idx = a.find(b) if op == "find" else a.rfind(b)
        check(op + ".found", int(r[0]), int(idx >= 0), ctx)
        if idx >= 0:
            check(op + ".index", digits_to_int(r[1:]), idx, ctx)
    elif op == "upper":
        check(op, dec_str(ops.to_upper(ea)), a.upper(), ctx)
    elif op == "lower":
        check(op, dec_str(ops.to_lower(ea)), a.lower(), ctx)
    elif op == "trim_start":
        check(op, dec_str(ops.trim_start(ea)), a.lstrip(WS), ctx)
    elif op == "trim_end":
        check(op, dec_str(ops.trim_end(ea)), a.rstrip(WS), ctx)
    elif op == "strip":
        check(op, dec_str(ops.strip(ea)), a.strip(WS), ctx)
    elif op == "replace":
        if len(b) == 0:
            continue
        to = bytes(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), size=len(b)))
        if clear:
            got = dec_str(ops.replace(ea, b, to))
        else:
            got = dec_str(ops.replace(ea, enc(b, len(b)), enc(to, len(b))))
        check(op, got, a.replace(b, to), ctx + (to,))
    elif op == "replace_general":
        # any lengths; clear operands (incl. the empty pattern) or encrypted zero padded ones
        to = bytes(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), size=int(rng.integers(0, 4))))
        if not clear and len(b) == 0:
            continue        # an encrypted empty pattern replaces nothing by definition (fhestr.h)
        want = a.replace(b, to)
        out_cap = max(1, len(want) + int(rng.integers(0, 2)))
        if clear:
            got = dec_str(ops.replace(ea, b, to, out_cap=out_cap))
        else:
            got = dec_str(ops.replace(ea, eb, enc(to, max(1, len(to) + int(rng.integers(0, 2)))), out_cap=out_cap))
        check(op, got, want, ctx + (to, out_cap))
    elif op == "len":
        check(op, digits_to_int(dec(ops.len(ea))), len(a), ctx)
    elif op == "is_empty":
        check(op, int(dec(ops.is_empty(ea))[0]), int(len(a) == 0), ctx)
    elif op == "concat":
        check(op, dec_str(ops.concat(ea, rhs)), a + b, ctx)
    elif op == "repeat":
        n = int(rng.integers(1, 4))
        check(op, dec_str(ops.repeat(ea, n)), a * n, ctx + (n,))
    elif op in ("strip_prefix", "strip_suffix"):
        bit, out = getattr(ops, op)(ea, rhs)          # clear or encrypted (padded) pattern
        had = a.startswith(b) if op == "strip_prefix" else a.endswith(b)
        want = (a[len(b):] if op == "strip_prefix" else a[:len(a) - len(b)]) if had else a
        check(op + ".bit", int(dec(bit)[0]), int(had), ctx)
        check(op + ".str", dec_str(out), want, ctx)
    elif op == "split":
        # one operation of the family; clear or encrypted (zero padded) separator, often a part capacity that cuts
        name = str(rng.choice(SPLIT_OPS))
        if len(b) == 0:
            continue        # a clear empty separator is refused, an encrypted one separates nothing (fhestr.h)
        max_parts = int(rng.integers(1, 5))
        part_cap = int(rng.integers(1, cap + 1)) if rng.random() < 0.4 else None
        res = getattr(ops, name)(ea, rhs, part_cap) if name in ONCE else getattr(ops, name)(ea, rhs, max_parts, part_cap)
        flat = np.concatenate([np.asarray(res.count).reshape(-1, p.big_size)] + list(res.parts))
        got = decode_split(name, dec(flat), p.msg_mod, max_parts, part_cap or cap)
        check(name, got, split_ref(name, a, b, max_parts, part_cap=part_cap), ctx + (max_parts, part_cap))
    elif op == "split_ws":
        max_parts = int(rng.integers(1, 5))
        res = ops.split_ascii_whitespace(ea, max_parts)
        flat = np.concatenate([np.asarray(res.count).reshape(-1, p.big_size)] + list(res.parts))
        check(op, decode_split("split_ascii_whitespace", dec(flat), p.msg_mod, max_parts, cap),
              split_ref("split_ascii_whitespace", a, None, max_parts), ctx + (max_parts,))
    elif op == "replacen":
        if len(b) == 0:
            continue
        to = bytes(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), size=int(rng.integers(0, 4))))
        n = int(rng.integers(0, 4))
        want = a.replace(b, to, n)
        out_cap = max(1, len(want) + int(rng.integers(0, 2)))
        if clear:
            got = dec_str(ops.replacen(ea, b, to, n, out_cap=out_cap))
        else:
            got = dec_str(ops.replacen(ea, eb, enc(to, max(1, len(to) + int(rng.integers(0, 2)))), n, out_cap=out_cap))
        check(op, got, want, ctx + (to, n, out_cap))
    elif op == "slice":
        # take / skip / split_at / char_at / insert at a clear position, or at an encrypted one with a bound below, at or above
        # the capacity: n in 0 .. n_max + 2 (what the digits of n_max cannot hold is left out); t = b, encrypted or clear
        name = str(rng.choice(["take", "skip", "split_at", "char_at", "insert"]))
        slices += 1
        n_max = int(rng.integers(1, 2 * cap + 2)) if rng.random() < 0.6 else None
        n = int(rng.integers(0, (n_max or cap) + 3))
        out_cap = int(rng.integers(1, cap + 4)) if name != "char_at" and rng.random() < 0.4 else None
        at = n
        if n_max is not None:
            n = min(n, p.msg_mod ** fhestr.count_input_digits(P, n_max) - 1)
            at = fhestr.EncryptedCount(ck.encrypt_many(fhestr.encode_count(P, n, n_max)), n_max)
        args = (ea, at, rhs) if name == "insert" else (ea, at)
        got = getattr(ops, name)(*args) if out_cap is None else getattr(ops, name)(*args, out_cap=out_cap)
        flat = np.concatenate([np.asarray(x).reshape(-1, p.big_size) for x in got]) if isinstance(got, tuple) else got
        cap_out = out_cap or cap + ((len(b) if clear else b_cap) if name == "insert" else 0)
        check(op + "." + name, decode_slice(name, dec(flat), p.msg_mod, cap_out),
              slice_ref(name, a, n, n_max, cap_out, b if name == "insert" else b""), ctx + (n, n_max, out_cap))
    elif op == "combine":
        # bit logic on k random bits, a select between a and b (encrypted or clear, any output capacity), or a count operation on
        # two counts with random bounds (the second one encrypted or clear): operands above their bound included
        combines += 1
        kind = str(rng.choice(["bits", "select", "count", "count"]))
        enc_bit = lambda v: ck.encrypt_many(np.array([v], dtype=np.uint64))
        msgs = lambda ct: [int(m) for m in dec(ct)]
        if kind == "bits":
            name = str(rng.choice(["and", "or", "xor", "not"]))
            bits = [int(v) for v in rng.integers(0, 2, size=int(rng.integers(1 if name == "not" else 2, 20)))]
            got = msgs(getattr(ops, "bit_" + name)(*[enc_bit(v) for v in bits]))
            check(op + "." + name, got if name == "not" else decode_bit(got), bits_ref(name, bits), ctx + (bits,))
        elif kind == "select":
            c = int(rng.integers(0, 2))
            out_cap = int(rng.integers(1, cap + 4)) if rng.random() < 0.5 else None
            cap_out = out_cap or max(cap, len(b) if clear else b_cap, 1)
            got = ops.select(enc_bit(c), ea, rhs) if out_cap is None else ops.select(enc_bit(c), ea, rhs, out_cap=out_cap)
            check(op + ".select", decode_string(msgs(got), p.msg_mod, cap_out), select_ref(c, a, b, cap_out), ctx + (c, out_cap))
        else:
            name = str(rng.choice(COUNT_OPS))
            a_max, b_max = int(rng.integers(1, 70)), int(rng.integers(1, 70))
            holds = lambda n_max: p.msg_mod ** fhestr.count_input_digits(P, n_max) - 1
            x, y = int(rng.integers(0, min(a_max + 3, holds(a_max)) + 1)), int(rng.integers(0, min(b_max + 3, holds(b_max)) + 1))
            count = lambda v, n_max: fhestr.EncryptedCount(ck.encrypt_many(fhestr.encode_count(P, v, n_max)), n_max)
            got = getattr(ops, "count_" + name)(count(x, a_max), y if clear else count(y, b_max))
            want = count_ref(name, x, a_max, y, None if clear else b_max)
            if name in ("add", "sub"):
                got = decode_digits(msgs(got.digits), p.msg_mod, count_bound(name, a_max, y if clear else b_max))
            else:
                got = decode_bit(msgs(got))
            check(op + ".count_" + name, got, want, ctx + (x, a_max, y, b_max))
    elif op.endswith("_encn"):
        # an encrypted count: n in 0 .. n_max + 1 (what the digits of n_max cannot hold is left out)
        n_max = int(rng.integers(1, 6))
        n = min(int(rng.integers(0, n_max + 2)), p.msg_mod ** fhestr.count_input_digits(P, n_max) - 1)
        count = fhestr.EncryptedCount(ck.encrypt_many(fhestr.encode_count(P, n, n_max)), n_max)
        if op == "repeat_encn":
            check(op, dec_str(ops.repeat(ea, count)), repeat_ref(a, n, n_max), ctx + (n, n_max))
            continue
        if clear and len(b) == 0:
            continue        # a clear empty pattern is refused; an encrypted one selects / separates nothing
        if op == "replacen_encn":
            to = bytes(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), size=int(rng.integers(0, 4))))
            want = replacen_ref(a, b, to, n, n_max)
            out_cap = max(1, len(want) + int(rng.integers(0, 2)))
            e_to = to if clear else enc(to, max(1, len(to) + int(rng.integers(0, 2))))
            check(op, dec_str(ops.replacen(ea, rhs, e_to, count, out_cap=out_cap)), want, ctx + (to, n, n_max, out_cap))
        else:
            name = op[:-len("_encn")]
            part_cap = int(rng.integers(1, cap + 1)) if rng.random() < 0.4 else None
            res = getattr(ops, name)(ea, rhs, count, part_cap)
            flat = np.concatenate([np.asarray(res.count).reshape(-1, p.big_size)] + list(res.parts))
            check(op, decode_split("splitn", dec(flat), p.msg_mod, n_max, part_cap or cap),
                  splitn_ref(name, a, b, n, n_max, part_cap=part_cap), ctx + (n, n_max, part_cap))
print(f"fuzz: {N_CASES} cases ({slices} of them slices, {combines} combining results), {fails} mismatches")
sys.exit(1 if fails else 0)
