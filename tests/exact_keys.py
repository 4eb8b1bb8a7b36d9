"""Server keys checked from the DEFINITION of an LWE / GLWE / GGSW encryption (DESIGN.md section 2 layouts): subtract from
every body what the masks, the secret keys and the plaintext rule put there; what is left is the noise, and that has to
be an honest centred normal sample of the parameter set's deviation, drawn from streams that never repeat.

Plain numpy on uint64 with wrapping arithmetic, no floating point in the residuals.  Imports neither the engine nor the
oracle's key generator: word-for-word tests against either compare a formula with a copy of itself; this file restates the
reference's rules (lwe_keyswitch_key_generation.rs:65-130, ggsw_encryption.rs:300-331,
lwe_multi_bit_bootstrap_key_generation.rs:401-427) and nothing of the product's."""
import math

import numpy as np

U64 = np.uint64


def _u64(a):
    return np.ascontiguousarray(a, dtype=U64)


def ksk_noise(p, ksk, glwe_sk, small_sk):
    """int64[kN, ks_level]: body - sum_j mask_j small_sk_j - (glwe_sk_i << (64 - ks_base_log (ks_level - it))) of row (i, it)
    of a keyswitch key [kN][ks_level, level ks_level first][n + 1]."""
    kN, L, n = p.k * p.N, p.ks_level, p.n
    rows = _u64(ksk).reshape(kN, L, n + 1)
    s = _u64(small_sk).reshape(n)
    g = _u64(glwe_sk).reshape(kN)
    shift = np.array([64 - p.ks_base_log * (L - it) for it in range(L)], dtype=U64)
    with np.errstate(over="ignore"):
        dot = (rows[:, :, :n] * s).sum(axis=2, dtype=U64)
        return (rows[:, :, n] - dot - (g[:, None] << shift[None, :])).view(np.int64)


def ggsw_bits(p, small_sk, G):
    """Plaintext bit of every GGSW of the bootstrapping key.  Classic PBS (G <= 1): the small key's bits.  Multi-bit: group
    t holds key bits s_0 .. s_{G-1} = small_sk[t G : (t + 1) G] and 2^G GGSWs; GGSW `sel` of the group encrypts the product
    over b of s_b where bit G-1-b of sel is set and of 1 - s_b where it is clear (combine_key_bits,
    lwe_multi_bit_bootstrap_key_generation.rs:401-427: bit_position = len - (bit_idx + 1), key_bit ^ inversion_bit)."""
    s = _u64(small_sk).reshape(p.n)
    if G <= 1:
        return s.copy()
    assert p.n % G == 0
    out = np.zeros((p.n // G, 1 << G), dtype=U64)
    for t in range(p.n // G):
        for sel in range(1 << G):
            prod = 1
            for b in range(G):
                bit = int(s[t * G + b])
                prod *= bit if (sel >> (G - 1 - b)) & 1 else 1 - bit
            out[t, sel] = prod
    return out.reshape(-1)


def negacyclic_by_binary_key(A, S):
    """A (rows, N) uint64 times the binary polynomial S (N,) mod (X^N + 1, 2^64): the signed sum of the rotated copies of A
    that S selects, result[c] = sum_{t <= c} A[c - t] - sum_{t > c} A[c + N - t] over the t with S[t] = 1."""
    A = _u64(A)
    N = A.shape[1]
    S = _u64(S).reshape(N)
    assert int(S.max(initial=0)) <= 1
    with np.errstate(over="ignore"):
        ext = np.concatenate([U64(0) - A, A], axis=1)      # ext[:, N + j] = A[:, j], ext[:, j] = -A[:, j]
        acc = np.zeros_like(A)
        for t in np.flatnonzero(S):
            acc += ext[:, N - t:2 * N - t]
    return acc


def bsk_noise(p, bsk, glwe_sk, bits, ggsw_indices=None):
    """int64[len, L, k+1, N]: body - sum_q A_q * S_q - plaintext of every GLWE row of the chosen GGSWs of a bootstrapping key
    [n_ggsw][L, level 1 first][k+1 rows][k+1 polynomials][N].  Plaintext (ggsw_encryption.rs:300-331), m the GGSW's bit,
    level l 1-based: row r < k carries -m S_r 2^(64 - base_log l), row k carries +m 2^(64 - base_log l) on coefficient 0."""
    k, N, L = p.k, p.N, p.pbs_level
    bits = _u64(bits).reshape(-1)
    key = _u64(bsk).reshape(bits.size, L, k + 1, k + 1, N)
    idx = np.arange(bits.size) if ggsw_indices is None else np.asarray(ggsw_indices, dtype=np.int64)
    S = _u64(glwe_sk).reshape(k, N)
    sel = key[idx]                                           # (len, L, k+1, k+1, N)
    flat = sel.reshape(-1, k + 1, N)
    with np.errstate(over="ignore"):
        res = flat[:, k, :].copy()
        for q in range(k):
            res -= negacyclic_by_binary_key(flat[:, q, :], S[q])
        res = res.reshape(len(idx), L, k + 1, N)
        m = bits[idx]
        for l in range(1, L + 1):
            scale = m << U64(64 - p.pbs_base_log * l)        # m 2^(64 - base_log l), m in {0, 1}
            for r in range(k):
                res[:, l - 1, r, :] += scale[:, None] * S[r][None, :]        # minus (-m S_r scale)
            res[:, l - 1, k, 0] -= scale
    return res.view(np.int64)


_ERF = {1: math.erf(1 / math.sqrt(2)), 2: math.erf(2 / math.sqrt(2)), 3: math.erf(3 / math.sqrt(2))}


def normal_stats(e, std):
    """The statistics normal_checks bounds, as {name: (value, bound)}; the variance ratio is reported around 1."""
    e = np.asarray(e, dtype=np.int64).reshape(-1)
    M = e.size
    sigma = float(std) * 2.0 ** 64
    x = e.astype(np.float64)
    out = {"mean/sigma": (abs(x.mean()) / sigma, 6.0 / math.sqrt(M)),
           "var/sigma^2 - 1": (abs((x * x).mean() / sigma ** 2 - 1.0), 6.0 * math.sqrt(2.0 / M))}
    ax = np.abs(x)
    for c, q in _ERF.items():
        out[f"fraction within {c} sigma - {q:.6f}"] = (abs(float((ax <= c * sigma).mean()) - q), 6.0 * math.sqrt(q * (1 - q) / M))
    out["max|e|/sigma"] = (float(ax.max()) / sigma, 7.5)
    return out


def variance_ratio(e, std):
    x = np.asarray(e, dtype=np.int64).reshape(-1).astype(np.float64)
    return float((x * x).mean()) / (float(std) * 2.0 ** 64) ** 2


def normal_checks(e, std, name):
    """`e`: M signed noise samples that should be N(0, sigma^2) rounded to integers, sigma = std 2^64.  Every bound is six
    standard errors of its statistic under that law (mean: sigma / sqrt M; variance: sigma^2 sqrt(2 / M), about zero as
    the law is centred; a fraction q: sqrt(q (1 - q) / M)), so a correct sampler fails one of the five with probability
    below 5 * 2e-9, and max |e| < 7.5 sigma fails with probability M * 6.4e-14.  Nothing here was measured."""
    sigma = float(std) * 2.0 ** 64
    if not sigma >= 64.0:
        raise ValueError(f"{name}: sigma = {sigma:.3g} < 2^6: the integer rounding of the samples would show in the statistics")
    M = np.asarray(e).size
    for stat, (value, bound) in normal_stats(e, std).items():
        ok = value < bound if stat.startswith("max") else value <= bound
        assert ok, f"{name}: {stat} = {value:.6g} exceeds {bound:.6g} (M = {M}, sigma = 2^{math.log2(sigma):.2f})"


def repeat_bound(M, sigma):
    """Upper bound on the number of equal PAIRS among M honest samples of N(0, sigma^2) rounded to integers.  With p_v the
    probability of value v, sum p^2 = 1 / (2 sigma sqrt pi) and sum p^3 = 1 / (2 pi sigma^2 sqrt 3) (sigma >= 2^6: the sums
    are their integrals); the pair count C has mean lam = M (M - 1) / 2 * sum p^2 -- the M^2 / sigma law, 0.141 M^2 / sigma
    -- and variance lam (1 - sum p^2) + M (M - 1) (M - 2) (sum p^3 - (sum p^2)^2).  Bound: lam + 6 sqrt(var) + 10; the
    ten covers the Poisson regime lam < 1, where P(C >= 11) <= lam^11 / 11! < 3e-8."""
    p2 = 1.0 / (2.0 * sigma * math.sqrt(math.pi))
    p3 = 1.0 / (2.0 * math.pi * sigma * sigma * math.sqrt(3.0))
    lam = M * (M - 1) / 2.0 * p2
    var = lam * (1.0 - p2) + M * (M - 1.0) * (M - 2.0) * (p3 - p2 * p2)
    return lam, lam + 6.0 * math.sqrt(var) + 10.0


def _equal_pairs(values):
    _, counts = np.unique(np.asarray(values).reshape(-1), return_counts=True)
    counts = counts.astype(np.int64)
    return int((counts * (counts - 1) // 2).sum())


def distinct_streams(ksk, bsk, p, n_ggsw=None, ksk_res=None, bsk_res=None):
    """Every key row draws from a stream of its own: the first mask word of every keyswitch-key row and of every GLWE row of
    the bootstrapping key, all together, are pairwise distinct (R honest 64-bit words collide with probability
    R^2 / 2^65: below 1e-9 up to R = 1.8e5 rows, the largest key here).  With the residuals given, no noise value repeats
    more often than repeat_bound allows for honest samples."""
    k, N, L = p.k, p.N, p.pbs_level
    n_ggsw = p.n if n_ggsw is None else n_ggsw
    first = np.concatenate([_u64(ksk).reshape(-1, p.n + 1)[:, 0],
                            _u64(bsk).reshape(n_ggsw * L * (k + 1), (k + 1) * N)[:, 0]])
    pairs = _equal_pairs(first)
    assert pairs == 0, f"{pairs} pairs of key rows start with the same mask word: they read the same stream"
    for name, res, std in (("ksk", ksk_res, p.lwe_std), ("bsk", bsk_res, p.glwe_std)):
        if res is None:
            continue
        M = np.asarray(res).size
        lam, bound = repeat_bound(M, std * 2.0 ** 64)
        pairs = _equal_pairs(res)
        assert pairs <= bound, f"{name}: {pairs} equal pairs among {M} noise values, honest samples give {lam:.4g} (bound {bound:.4g})"
