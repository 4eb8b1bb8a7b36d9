"""The packing keyswitch written from its definition, in exact integers (test infrastructure; independent of oracle/ and
of the engine).  For LWE number d of a group of at most N big-key LWEs (a_0 .. a_{kN-1}, b),

    T_d[p][c]   = [p == k and c == 0] * b_d  -  sum_{i, lv} digit(a_i, lv) * PKSK[i][lv][p][c]          (mod 2^64)
    out[p][c'] += T_d[p][c]     where c + d = c' (< N)
    out[p][c'] -= T_d[p][c]     where c + d = c' + N              (multiplication by X^d in Z[X] / (X^N + 1))

(core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187,297-380) with the signed digits of the closest representable
value of a_i, level L first, exactly as in the LWE keyswitch (exact_keyswitch.py).  Key layout
[kN][level, level L first][k+1][N]; LWE j of a longer list goes to GLWE j // N, coefficient j % N.

Two forms:
  * pack_int: Python integers only, for tiny shapes;
  * ExactPacking: T for whole batches by ExactKeyswitch's float64 16-bit-limb products (every partial sum an integer below
    2^53, asserted there) over (k+1) N output columns, then the rotation and the sum in wrapping uint64."""
from types import SimpleNamespace

import numpy as np

from exact_keyswitch import EDGE_KEY_WORDS, ExactKeyswitch, decompose_int, edge_big_cts

U64 = np.uint64
M64 = (1 << 64) - 1


def as_keyswitch_shape(params, pp):
    """The packing product seen as an LWE keyswitch: k N inputs, (k+1) N output columns, the packing decomposition."""
    base_log, level = pp
    return SimpleNamespace(k=params.k, N=params.N, n=(params.k + 1) * params.N - 1, ks_base_log=base_log, ks_level=level)


# ---- the definition, Python integers ---------------------------------------------------------------------------------------

def pack_int(params, pp, pksk, cts):
    """cts [count, k N + 1] -> [ceil(count / N), k + 1, N], Python integers throughout."""
    k, N = params.k, params.N
    base_log, level = pp
    in_dim, glwe_len = k * N, (k + 1) * N
    pksk = np.asarray(pksk, dtype=U64).reshape(in_dim * level, glwe_len)
    cts = np.asarray(cts, dtype=U64).reshape(-1, in_dim + 1)
    out = [[0] * glwe_len for _ in range(-(-len(cts) // N))]
    for j, ct in enumerate(cts.tolist()):
        t = [0] * glwe_len
        t[k * N] = ct[in_dim]
        for i in range(in_dim):
            for lv, dg in enumerate(decompose_int(ct[i], base_log, level)):
                if dg:
                    row = pksk[i * level + lv].tolist()
                    for c in range(glwe_len):
                        t[c] -= dg * row[c]
        o, d = out[j // N], j % N
        for p in range(k + 1):
            for c in range(N):
                if c + d < N:
                    o[p * N + c + d] += t[p * N + c]
                else:
                    o[p * N + c + d - N] -= t[p * N + c]
    return np.array([[v & M64 for v in o] for o in out], dtype=U64).reshape(-1, k + 1, N)


# ---- the same as exact float64 limb products, then rotate and sum -------------------------------------------------------------

class ExactPacking:
    """ExactPacking(params, pp, pksk)(cts [count, k N + 1]) -> [ceil(count / N), k + 1, N]."""

    def __init__(self, params, pp, pksk):
        self.k, self.N = params.k, params.N
        self.ks = ExactKeyswitch(as_keyswitch_shape(params, pp), pksk)

    def rows(self, cts):
        """T_d of every LWE: [count, k + 1, N]."""
        k, N = self.k, self.N
        cts = np.asarray(cts, dtype=U64).reshape(-1, k * N + 1)
        t = self.ks(cts)                       # the keyswitch form adds the body at its last column: move it to (k, 0)
        with np.errstate(over="ignore"):
            t[:, -1] -= cts[:, k * N]
            t[:, k * N] += cts[:, k * N]
        return t.reshape(len(cts), k + 1, N)

    def __call__(self, cts):
        k, N = self.k, self.N
        t = self.rows(cts)
        out = np.zeros((-(-len(t) // N), k + 1, N), dtype=U64)
        with np.errstate(over="ignore"):
            for j in range(len(t)):
                d = j % N
                rot = np.roll(t[j], d, axis=1)
                rot[:, :d] = U64(0) - rot[:, :d]                # the coefficients that wrapped past X^N = -1
                out[j // N] += rot
        return out


def pack_exact(params, pp, pksk, cts):
    return ExactPacking(params, pp, pksk)(cts)


# ---- edge inputs --------------------------------------------------------------------------------------------------------------

def edge_pack_cts(params, pp, rng, count):
    """edge_big_cts under the packing decomposition: the first rows sit on the decomposer's edges, the rest are uniform."""
    return edge_big_cts(as_keyswitch_shape(params, pp), rng, count)


def edge_pksk(params, pp, rng):
    """Packing key [k N * level, k + 1, N], uniform words except, in EVERY polynomial: columns j < 8 and N - 16 + j hold
    EDGE_KEY_WORDS[j] in every row (with the pos / neg_max rows of edge_big_cts the accumulator column sits at its
    extreme), columns 8 + j and N - 8 + j hold them in every other row.  Both ends of a polynomial, so that the extreme
    columns meet the wrap at X^N for small and for large degrees."""
    base_log, level = pp
    k, N = params.k, params.N
    key = rng.integers(0, 2**64, size=(k * N * level, k + 1, N), dtype=U64)
    for j, w in enumerate(EDGE_KEY_WORDS):
        key[:, :, j] = w
        key[j % 2::2, :, 8 + j] = w
        key[:, :, N - 16 + j] = w
        key[j % 2::2, :, N - 8 + j] = w
    return key


# ---- large keys: sparse masks -----------------------------------------------------------------------------------------------------

def sparse_case(params, pp, count, n_elements=48, seed=0):
    """(key, cts, exact result) for shapes whose whole key is too large to multiply: `count` LWEs whose masks are zero
    except at `n_elements` positions (the first and last element, the ends of 16-slot groups, random ones), which carry
    the edge values in turn and uniform words.  A zero element has zero digits, so only the key rows of those positions
    matter: the key is allocated zeroed and those rows alone are drawn; the result is the definition over these rows,
    T_d = (0, .., b_d at (k, 0)) - sum digit * row in wrapping uint64, then the rotation and the sum."""
    from exact_keyswitch import edge_mask_values
    base_log, level = pp
    k, N = params.k, params.N
    in_dim, glwe_len = k * N, (k + 1) * N
    rng = np.random.default_rng([N, k, base_log, level, count, seed])
    epg = 16 // level
    fixed = [0, 1, epg - 1, epg, 2 * epg - 1, 2 * epg, in_dim // 2, in_dim - 2 * epg, in_dim - epg - 1, in_dim - 2, in_dim - 1]
    pos = np.unique(np.concatenate([np.array(fixed), rng.integers(0, in_dim, size=n_elements - len(fixed))]))
    key = np.zeros((in_dim * level, k + 1, N), dtype=U64)
    rows = (pos[:, None] * level + np.arange(level)[None, :]).reshape(-1)
    key[rows] = rng.integers(0, 2**64, size=(len(rows), k + 1, N), dtype=U64)
    for j, w in enumerate(EDGE_KEY_WORDS):                       # extreme columns at both ends of every polynomial
        key[rows, :, j] = w
        key[rows, :, N - 8 + j] = w
    edge = list(edge_mask_values(base_log, level).values())
    cts = np.zeros((count, in_dim + 1), dtype=U64)
    cts[:, pos] = rng.integers(0, 2**64, size=(count, len(pos)), dtype=U64)
    for b in range(min(count, len(edge))):
        cts[b, pos] = edge[b]                                   # a row of every edge value
    cts[:, in_dim] = rng.integers(0, 2**64, size=count, dtype=U64)
    out = np.zeros((-(-count // N), k + 1, N), dtype=U64)
    with np.errstate(over="ignore"):
        for j in range(count):
            t = np.zeros((k + 1, N), dtype=U64)
            t[k, 0] = cts[j, in_dim]
            for e, i in enumerate(pos):
                for lv, dg in enumerate(decompose_int(int(cts[j, i]), base_log, level)):
                    if dg:
                        t -= U64(dg & M64) * key[i * level + lv]
            d = j % N
            rot = np.roll(t, d, axis=1)
            rot[:, :d] = U64(0) - rot[:, :d]
            out[j // N] += rot
    return key, cts, out
