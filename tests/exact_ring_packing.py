"""Ring packing written from its definition, in Python integers with schoolbook negacyclic products (test infrastructure;
independent of the engine and of any transform).  All ciphertext arithmetic mod 2^64; the phase is B - sum_q A_q S_q.

    leaf      w' = (w + N/2) >> log2 N for every word of the LWE; A_q[0] = a'[qN], A_q[i] = -a'[qN + N - i], B[0] = b'
    autoKS_l  t = 2^l + 1, sigma_t(P)(X) = P(X^t) in Z[X] / (X^N + 1):
              (0, .., 0, sigma_t(B)) - sum_q sum_it digit_it(sigma_t(A_q)) (*) AK[l][q][it]
    pack      pack(0, {ct}) = ct;  e = pack(l - 1, even-indexed), o = pack(l - 1, odd-indexed), s = N / 2^l:
              pack(l, cts) = (e + X^s o) + autoKS_l(e - X^s o);  an absent leaf is the zero ciphertext, a node with no
              leaf costs nothing
    key       [log2 N][k][level, level L first][k + 1][N]: AK[l][q][it] encrypts S_q(X^t) << (64 - base_log (L - it))

LWE j of a longer list goes to GLWE j // N, coefficient j % N.  The digits are exact_keyswitch.decompose_int's (level L
first).  The recursion below is the definition as stated; the library walks the same tree level by level."""
import numpy as np

from exact_keyswitch import decompose_int

M64 = (1 << 64) - 1
P = 4293918721          # 2^32 - 2^20 + 1


def negacyclic(a, b):
    """a (*) b in Z[X] / (X^N + 1), Python integers, no reduction."""
    N = len(a)
    out = [0] * N
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < N:
                    out[i + j] += x * y
                else:
                    out[i + j - N] -= x * y
    return out


def automorphism(poly, t):
    """P(X^t): coefficient j goes to j t mod 2N, negated past N."""
    N = len(poly)
    out = [0] * N
    for j, v in enumerate(poly):
        e = j * t % (2 * N)
        if e < N:
            out[e] = v
        else:
            out[e - N] = -v
    return out


def shift(poly, s):
    """X^s P."""
    N = len(poly)
    return [poly[j - s] if j >= s else -poly[j - s + N] for j in range(N)]


def leaf(ct, k, N):
    logN = N.bit_length() - 1
    w = [((int(x) + N // 2) & M64) >> logN for x in ct]
    glwe = []
    for q in range(k):
        glwe.append([w[q * N]] + [(-w[q * N + N - i]) & M64 for i in range(1, N)])
    glwe.append([w[k * N]] + [0] * (N - 1))
    return glwe


def auto_ks(ct, level, key, k, N, pair):
    """ct: k + 1 polynomials; key: this tree level's [k][L][k + 1][N] as nested lists."""
    base_log, L = pair
    t = (1 << level) + 1
    out = [[0] * N for _ in range(k)] + [automorphism(ct[k], t)]
    for q in range(k):
        perm = [v & M64 for v in automorphism(ct[q], t)]
        digits = [decompose_int(v, base_log, L) for v in perm]
        for it in range(L):
            d = [dg[it] for dg in digits]
            for qo in range(k + 1):
                prod = negacyclic(d, key[q][it][qo])
                out[qo] = [a - b for a, b in zip(out[qo], prod)]
    return [[v & M64 for v in poly] for poly in out]


def pack_node(level, cts, key, k, N, pair):
    """cts: the node's leaves in list order, None where absent.  Returns the node's GLWE, or None if it holds no leaf."""
    if all(c is None for c in cts):
        return None
    if level == 0:
        return cts[0]
    e = pack_node(level - 1, cts[0::2], key, k, N, pair)
    o = pack_node(level - 1, cts[1::2], key, k, N, pair)
    s = N >> level
    zero = [[0] * N for _ in range(k + 1)]
    e = e if e is not None else zero
    xo = [shift(poly, s) for poly in o] if o is not None else zero
    plus = [[(a + b) & M64 for a, b in zip(pe, po)] for pe, po in zip(e, xo)]
    minus = [[(a - b) & M64 for a, b in zip(pe, po)] for pe, po in zip(e, xo)]
    ks = auto_ks(minus, level, key[level - 1], k, N, pair)
    return [[(a + b) & M64 for a, b in zip(pp, pk)] for pp, pk in zip(plus, ks)]


def ring_pack_int(params, pair, key, cts):
    """cts [count, k N + 1] -> [ceil(count / N), k + 1, N], Python integers throughout."""
    k, N = params.k, params.N
    logN = N.bit_length() - 1
    key = np.asarray(key, dtype=np.uint64).reshape(logN, k, pair[1], k + 1, N).tolist()
    cts = np.asarray(cts, dtype=np.uint64).reshape(-1, k * N + 1)
    out = []
    for at in range(0, len(cts), N):
        leaves = [leaf(ct, k, N) for ct in cts[at:at + N].tolist()]
        leaves += [None] * (N - len(leaves))
        out.append(pack_node(logN, leaves, key, k, N, pair))
    return np.array(out, dtype=np.uint64).reshape(-1, k + 1, N)


def keyswitch_count(N, count):
    """sum over the GLWEs of sum_{d < log2 N} min(2^d, c)."""
    total = 0
    for at in range(0, count, N):
        c = min(N, count - at)
        total += sum(min(1 << d, c) for d in range(N.bit_length() - 1))
    return total


def variance(params, pair):
    """What ring packing adds to a packed coefficient (torus = 1): (N^2 / 3) V_aks + the division's term."""
    base_log, L = pair
    N, kN = params.N, params.k * params.N
    v_aks = kN * L * (4.0**base_log + 2) / 12 * params.glwe_std**2 + kN / 2 / 12 * 4.0**(-base_log * L)
    return N * N / 3 * v_aks + N * N * kN / 24 * 2.0**-128


def prime_bound_ok(params, pair):
    return params.k * pair[1] * params.N * 128 * 2**(pair[0] - 1) < P // 2


def edge_key(params, pair, rng):
    """Uniform key words with extreme balanced-digit patterns (every plane -128, every plane 127, 0, a lone top bit) at
    both ends of every polynomial."""
    k, N = params.k, params.N
    logN = N.bit_length() - 1
    key = rng.integers(0, 2**64, size=(logN * k * pair[1], k + 1, N), dtype=np.uint64)
    edges = [0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0, 1 << 63]
    for j, w in enumerate(edges[:max(1, N // 4)]):
        key[:, :, j] = np.uint64(w)
        key[:, :, N - 1 - j] = np.uint64(w)
    return key
