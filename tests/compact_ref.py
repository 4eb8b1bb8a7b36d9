"""numpy restatement of the reference's compact public-key algorithms (tfhe-rs 0.5, eprint 2023/603), the yardstick of
tests/test_compact_pk.py and tests/test_gpu_compact_pk.py.  Wrapping uint64 arithmetic, schoolbook convolution (no FFT):

  conv(lhs, rhs)  slice_semi_reverse_negacyclic_convolution   core_crypto/algorithms/slice_algorithms.rs:610-659
  public key      b = conv(a, s) + e                          lwe_compact_public_key_generation.rs:15-50
  list            A = conv(a, r) + e1, body c = conv(b, r)[c] + e2[c] + pt[c]   lwe_encryption.rs:1837-1958
  container       all bin masks, then all bodies              entities/lwe_compact_ciphertext_list.rs:41-63
  expansion       (A * X^(n - (c + 1)), body)                 lwe_compact_ciphertext_list_expansion.rs:12-58
"""
import numpy as np

U64 = np.uint64


def _u64(a):
    return np.ascontiguousarray(a, dtype=U64).reshape(-1)


def monomial_mul(poly, degree):
    """poly * X^degree in Z[X]/(X^n + 1), 0 <= degree < n (polynomial_wrapping_monic_monomial_mul_assign)."""
    poly = _u64(poly)
    n = poly.size
    out = np.empty(n, dtype=U64)
    out[degree:] = poly[:n - degree]
    out[:degree] = U64(0) - poly[n - degree:]
    return out


def conv(lhs, rhs):
    """lhs * reverse(rhs) in Z[X]/(X^n + 1): the product of the two polynomials term by term."""
    lhs, rhs = _u64(lhs), _u64(rhs)
    n = lhs.size
    assert rhs.size == n
    rev = rhs[::-1]
    out = np.zeros(n, dtype=U64)
    with np.errstate(over="ignore"):
        for m in range(n):
            if rev[m]:
                out += rev[m] * monomial_mul(lhs, m)
    return out


def list_len(n, count):
    return -(-count // n) * n + count


def public_key_body(a, s, e):
    with np.errstate(over="ignore"):
        return conv(a, s) + _u64(e)


def encrypt_list(a, b, r_bins, e1_bins, e2, plaintexts):
    """r_bins, e1_bins: (bins, n); e2, plaintexts: (count,).  Returns the container."""
    a, b, pts, e2 = _u64(a), _u64(b), _u64(plaintexts), _u64(e2)
    n, count = a.size, pts.size
    bins = -(-count // n)
    out = np.zeros(list_len(n, count), dtype=U64)
    with np.errstate(over="ignore"):
        for t in range(bins):
            lo, hi = t * n, min(count, (t + 1) * n)
            out[t * n:(t + 1) * n] = conv(a, r_bins[t]) + _u64(e1_bins[t])
            out[bins * n + lo:bins * n + hi] = conv(b, r_bins[t])[:hi - lo] + e2[lo:hi] + pts[lo:hi]
    return out


def expand(n, clist, count):
    """(count, n + 1) big LWEs [a_0 .. a_{n-1}, b]."""
    clist = _u64(clist)
    bins = -(-count // n)
    assert clist.size == list_len(n, count)
    out = np.zeros((count, n + 1), dtype=U64)
    for i in range(count):
        c = i % n
        out[i, :n] = monomial_mul(clist[(i // n) * n:(i // n + 1) * n], n - (c + 1))
        out[i, n] = clist[bins * n + i]
    return out


def phases(cts, s):
    """body - <mask, s> of every row, s binary."""
    cts = np.asarray(cts, dtype=U64)
    s = _u64(s)
    with np.errstate(over="ignore"):
        return cts[:, -1] - cts[:, :-1][:, s == 1].sum(axis=1, dtype=U64)
