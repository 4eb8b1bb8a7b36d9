"""An exact-integer programmable bootstrap in numpy, fast enough for N = 32768 (test infrastructure).

The C oracle's exact path (oracle/tfhe_oracle.c: orc_pbs_exact) multiplies polynomials the schoolbook way, N^2 per
product: seconds per PBS at N = 32768.  Here a negacyclic product  digits (|d| < 2^15)  x  key words (u64)  mod
(X^N + 1, 2^64) is taken limb by limb: the key in eight 8-bit limbs, each limb's product an f64 FFT whose values stay
below N * 2^15 * 2^8 = 2^38 -- the transform's rounding error is then < 2^-10, so rounding to the nearest integer is
EXACT -- and the limbs recombine in wrapping 64-bit integers.  Same algorithm as bootstrap.rs:242-331 / ggsw.rs:477-598
with the f64 external product replaced by exact arithmetic (last paragraph); pinned bit for bit
against orc_pbs_exact on small N (tests/test_exact_pbs.py)."""
import numpy as np

U64 = np.uint64


def _twist(N):
    return np.exp(1j * np.pi * np.arange(N) / N)


def negacyclic_mul_exact(digits, key, tw=None):
    """sum_j digits[j] * key[i - j] with X^N = -1, mod 2^64.  digits: int64 (|d| < 2^15), key: uint64."""
    N = len(key)
    tw = _twist(N) if tw is None else tw
    D = np.fft.fft(digits.astype(np.float64) * tw)
    out = np.zeros(N, dtype=U64)
    with np.errstate(over="ignore"):
        for t in range(8):
            limb = ((key >> U64(8 * t)) & U64(0xFF)).astype(np.float64)
            prod = np.fft.ifft(D * np.fft.fft(limb * tw)) * np.conj(tw)
            r = np.rint(prod.real)
            assert np.abs(prod.real - r).max() < 0.05 and np.abs(prod.imag).max() < 0.05      # exactness margin
            out += r.astype(np.int64).astype(U64) << U64(8 * t)
    return out


def decompose(x, base_log, level):
    """Signed digits of closest_representable(x), level `level` first (decomposer.rs:98-118, iter.rs:101-127): list of int64 arrays."""
    rep = base_log * level
    t = x >> U64(63 - rep)
    state = ((t + U64(1)) >> U64(1)) & U64((1 << rep) - 1)
    mask = U64((1 << base_log) - 1)
    digits = []
    for _ in range(level):
        res = state & mask
        state = state >> U64(base_log)
        carry = (((res - U64(1)) | state) & res) >> U64(base_log - 1)
        state = state + carry
        digits.append(res.astype(np.int64) - (carry.astype(np.int64) << base_log))
    return digits


def modulus_switch(x, logN):
    return int(((int(x) >> (64 - logN - 2)) + 1) >> 1)


def monomial_mul(poly, d, N):
    """poly * X^d, d in [0, 2N] (polynomial_algorithms.rs:425-490 / 315-354 via X^-d = X^(2N-d))."""
    d %= 2 * N
    rem, odd = d % N, (d // N) & 1
    out = np.roll(poly, rem)
    with np.errstate(over="ignore"):
        out[:rem] = U64(0) - out[:rem]
        if odd:
            out = U64(0) - out
    return out


def pbs_exact(params, bsk, ct_small, lut):
    """params: oracle Params; bsk: standard-domain key [n][level, level 1 first][k+1][k+1][N]; lut: [(k+1) N]."""
    n, k, N, bl, L = params.n, params.k, params.N, params.pbs_base_log, params.pbs_level
    logN = N.bit_length() - 1
    K1 = k + 1
    bsk = np.asarray(bsk, dtype=U64).reshape(n, L, K1, K1, N)
    tw = _twist(N)
    acc = np.asarray(lut, dtype=U64).reshape(K1, N).copy()
    b = modulus_switch(ct_small[n], logN)
    acc = np.stack([monomial_mul(p, 2 * N - b, N) for p in acc])          # X^{-ms(body)}
    with np.errstate(over="ignore"):
        for i in range(n):
            if int(ct_small[i]) == 0:
                continue                                                    # bootstrap.rs:281
            d = modulus_switch(ct_small[i], logN)
            ct1 = np.stack([monomial_mul(p, d, N) - p for p in acc])
            digs = [decompose(ct1[r], bl, L) for r in range(K1)]           # [row][it], it = 0 is level L
            for it in range(L):
                lvl = L - 1 - it                                            # index into "level 1 first"
                for r in range(K1):
                    for col in range(K1):
                        acc[col] += negacyclic_mul_exact(digs[r][it], bsk[i, lvl, r, col], tw)
    out = np.zeros(k * N + 1, dtype=U64)                                    # sample extraction at degree 0
    with np.errstate(over="ignore"):
        for p in range(k):
            out[p * N] = acc[p][0]
            out[p * N + 1: (p + 1) * N] = U64(0) - acc[p][:0:-1]
    out[k * N] = acc[k][0]
    return out


# ---- batched exact blind rotation over keys held as small integers ---------------------------------------------------
#
# A key word is a sum of terms  c << t  with c a small signed integer: the 8-bit limbs of a full-range u64 (t = 0, 8, ..
# 56), or a single term for the structured keys below.  digits (x) c then stays below L (k+1) N 2^(bl-1) 2^8 <= 2^44 on
# every shape of the engine, so ONE f64 negacyclic FFT product per term, rounded to the nearest integer, is exact (the
# rounding assertion in _spectral_product keeps that honest), and the term's contribution is that integer << t in
# wrapping 64-bit arithmetic.  Vectorised over a batch of LWEs: step i uses GGSW i of every LWE at once.

C_BITS = 8                     # structured keys: c in (-2^7, 2^7)
EXACT_BOUND_LOG2 = 56          # worst-case |f64 value| of a correct f64 external product, in units of 2^-64 (see structured_bsk)


def limb_terms(bsk):
    """A full-range u64 key as its eight 8-bit limbs: [(int64 array, shift)]."""
    bsk = np.asarray(bsk, dtype=U64)
    return [(((bsk >> U64(8 * j)) & U64(0xFF)).astype(np.int64), 8 * j) for j in range(8)]


def structured_shift(params, grouping=0):
    """Largest t <= 14 for which a correct f64 PBS of a key with words c << t (|c| < 2^7) is bit exact:
        * every product sum(digit * c) * 2^t lies on the 2^12 grid of the engine's from_torus (t >= 12), and
        * its worst case L (k+1) N 2^(bl-1) 2^7 2^t -- times (2^G - 1) 2 for a multi-bit key's combined GGSW -- stays
          below 2^56, so an f64 transform's rounding (relative 2^-53 times a few log N) stays far below half a grid step."""
    L, K1, N, bl = params.pbs_level, params.k + 1, params.N, params.pbs_base_log
    worst = np.log2(L * K1 * N) + (bl - 1) + (C_BITS - 1)
    if grouping:
        worst += np.log2(((1 << grouping) - 1) * 2)
    t = min(14, int(np.floor(EXACT_BOUND_LOG2 - worst)))
    assert t >= 12 and worst + t <= EXACT_BOUND_LOG2, (params.name, worst, t)
    return t


def structured_bsk(params, rng, grouping=0):
    """Bootstrapping key whose every word is c << t, c uniform in (-2^7, 2^7) stored as wrapping u64.  Returns
    (bsk [n_ggsw, L, k+1, k+1, N] u64, key terms [(c, t)], t); multi-bit keys hold n / G * 2^G GGSWs."""
    n_ggsw = params.n // grouping * (1 << grouping) if grouping else params.n
    t = structured_shift(params, grouping)
    lim = 1 << (C_BITS - 1)
    c = rng.integers(-lim + 1, lim, size=(n_ggsw, params.pbs_level, params.k + 1, params.k + 1, params.N), dtype=np.int64)
    return c.astype(U64) << U64(t), [(c, t)], t


def edge_small_cts(params, rng, count):
    """Small-key LWEs whose masks hold a_i = 0, values that modulus-switch to 0, 1, N, 2N - 1 and 2N, and random words;
    bodies include 0 and 2^64 - 1."""
    logN = params.N.bit_length() - 1
    q = 1 << (63 - logN)                                   # one step of the switched modulus 2N
    edges = [0, 1, q - 1, q, 2 * q, (params.N - 1) * q + q // 2, params.N * q, 2**63, 2**64 - q, 2**64 - 1]
    cts = rng.integers(0, 2**64, size=(count, params.n + 1), dtype=np.uint64)
    slots = [(b, i) for b in range(count) for i in range(params.n) if (i + b) % 3 == 0]      # a third of the mask: every edge in turn
    for j, (b, i) in enumerate(slots):
        cts[b, i] = edges[j % len(edges)]
    cts[0, params.n] = 0
    if count > 1:
        cts[1, params.n] = 2**64 - 1
    return cts


def monomial_mul_rows(polys, d):
    """polys[b] * X^d[b] for a batch: polys [B, ..., N] u64, d [B] in [0, 2N)."""
    N = polys.shape[-1]
    src = (np.arange(N)[None, :] - np.asarray(d, dtype=np.int64)[:, None]) % (2 * N)          # [B, N]
    neg = src >= N
    src = np.where(neg, src - N, src)
    shape = (polys.shape[0],) + (1,) * (polys.ndim - 2) + (N,)
    out = np.take_along_axis(polys, src.reshape(shape), axis=-1)
    with np.errstate(over="ignore"):
        return np.where(neg.reshape(shape), U64(0) - out, out)


def _spectral_product(D, Kspec, tw):
    """sum over (level, row) of digits (x) key, back to integers: D [B, L, K1, N] spectra of the digits, Kspec [(B,) L, K1, K1, N]
    spectra of one key term -> [B, K1, N] int64, exact."""
    S = np.einsum("blrn,blrcn->bcn" if Kspec.ndim == 5 else "blrn,lrcn->bcn", D, Kspec)
    prod = np.fft.ifft(S, axis=-1) * np.conj(tw)
    r = np.rint(prod.real)
    assert np.abs(prod.real - r).max() < 0.05 and np.abs(prod.imag).max() < 0.05      # exactness margin
    return r.astype(np.int64)


def _external_product(acc_in, terms_spec, tw, bl, L):
    """acc_in [B, K1, N] u64 decomposed and multiplied by the GGSW held as spectra of its terms: [(Kspec, t)] -> [B, K1, N] u64."""
    digs = decompose(acc_in, bl, L)                                        # L arrays [B, K1, N], level L first
    lvl_first = np.stack(digs[::-1], axis=1)                               # [B, L, K1, N], level 1 first (the key's order)
    D = np.fft.fft(lvl_first.astype(np.float64) * tw, axis=-1)
    out = np.zeros(acc_in.shape, dtype=U64)
    with np.errstate(over="ignore"):
        for Kspec, t in terms_spec:
            out += _spectral_product(D, Kspec, tw).astype(U64) << U64(t)
    return out


def _sample_extract(acc, k, N):
    B = acc.shape[0]
    out = np.zeros((B, k * N + 1), dtype=U64)
    with np.errstate(over="ignore"):
        for p in range(k):
            out[:, p * N] = acc[:, p, 0]
            out[:, p * N + 1: (p + 1) * N] = U64(0) - acc[:, p, :0:-1]
    out[:, k * N] = acc[:, k, 0]
    return out


def _start(params, cts, luts, lut_idx):
    N, K1, n = params.N, params.k + 1, params.n
    logN = N.bit_length() - 1
    cts = np.asarray(cts, dtype=U64).reshape(-1, n + 1)
    luts = np.asarray(luts, dtype=U64).reshape(-1, K1, N)
    idx = np.zeros(len(cts), dtype=np.int64) if lut_idx is None else np.asarray(lut_idx, dtype=np.int64)
    ms = np.vectorize(lambda x: modulus_switch(x, logN), otypes=[np.int64])
    acc = monomial_mul_rows(luts[idx], (2 * N - ms(cts[:, n])) % (2 * N))  # X^{-ms(body)}
    return cts, acc, ms


def pbs_exact_batch(params, terms, cts, luts, lut_idx=None):
    """Classic PBS of every row of cts (small-key LWEs) with LUT luts[lut_idx[b]], exact; the key as terms [(c, t)] of
    shape [n, L, k+1, k+1, N] (limb_terms(bsk) for any key).  Same algorithm as pbs_exact."""
    n, k, N, bl, L = params.n, params.k, params.N, params.pbs_base_log, params.pbs_level
    cts = np.asarray(cts, dtype=U64).reshape(-1, n + 1)
    if len(cts) > _chunk(params):
        return _chunked(pbs_exact_batch, params, (terms,), cts, luts, lut_idx)
    tw = _twist(N)
    cts, acc, ms = _start(params, cts, luts, lut_idx)
    with np.errstate(over="ignore"):
        for i in range(n):
            live = cts[:, i] != 0                                           # bootstrap.rs:281
            if not live.any():
                continue
            d = ms(cts[:, i]) % (2 * N)
            ct1 = monomial_mul_rows(acc, d) - acc
            spec = [(np.fft.fft(c[i].astype(np.float64) * tw, axis=-1), t) for c, t in terms]
            acc = np.where(live[:, None, None], acc + _external_product(ct1, spec, tw, bl, L), acc)
    return _sample_extract(acc, k, N)


def multi_bit_pbs_exact_batch(params, grouping, terms, cts, luts, lut_idx=None):
    """Multi-bit PBS (oracle/tfhe_oracle.c multi_bit_blind_rotate, exact branch) of every row of cts.  Per group: the
    combined GGSW  GGSW_0 + sum_{sel >= 1} X^{ms(sum of the selected mask elements)} GGSW_sel  (the selected sum taken
    in wrapping u64, then switched; selector bit G-1-b <-> mask element b of the group), then acc <- combined (x) acc.
    terms [(c, t)] of shape [n / G * 2^G, L, k+1, k+1, N]."""
    n, k, N, bl, L = params.n, params.k, params.N, params.pbs_base_log, params.pbs_level
    G = grouping
    cts = np.asarray(cts, dtype=U64).reshape(-1, n + 1)
    if len(cts) > _chunk(params):
        return _chunked(multi_bit_pbs_exact_batch, params, (grouping, terms), cts, luts, lut_idx)
    tw = _twist(N)
    cts, acc, ms = _start(params, cts, luts, lut_idx)
    B = len(cts)
    with np.errstate(over="ignore"):
        for grp in range(n // G):
            mask = cts[:, grp * G:(grp + 1) * G]
            spec = []
            for c, t in terms:
                comb = np.broadcast_to(c[grp << G], (B,) + c.shape[1:]).copy()
                for sel in range(1, 1 << G):
                    deg = np.zeros(B, dtype=U64)
                    for b in range(G):
                        if (sel >> (G - 1 - b)) & 1:
                            deg += mask[:, b]
                    sw = ms(deg) % (2 * N)
                    term = np.broadcast_to(c[(grp << G) + sel], (B,) + c.shape[1:])
                    comb += _monomial_mul_signed(term, sw)
                spec.append((np.fft.fft(comb.astype(np.float64) * tw, axis=-1), t))
            acc = _external_product(acc, spec, tw, bl, L)
    return _sample_extract(acc, k, N)


def _monomial_mul_signed(polys, d):
    """Signed-integer twin of monomial_mul_rows: polys [B, ..., N] int64."""
    N = polys.shape[-1]
    src = (np.arange(N)[None, :] - np.asarray(d, dtype=np.int64)[:, None]) % (2 * N)
    neg = src >= N
    src = np.where(neg, src - N, src)
    shape = (polys.shape[0],) + (1,) * (polys.ndim - 2) + (N,)
    out = np.take_along_axis(polys, np.broadcast_to(src.reshape(shape), polys.shape), axis=-1)
    return np.where(neg.reshape(shape), -out, out)


def _chunk(params):
    """LWEs per pass: the digit spectra of a pass stay near 32 MB."""
    return max(1, (1 << 21) // (params.pbs_level * (params.k + 1) * params.N))


def _chunked(fn, params, args, cts, luts, lut_idx):
    idx = np.zeros(len(cts), dtype=np.int64) if lut_idx is None else np.asarray(lut_idx, dtype=np.int64)
    step = _chunk(params)
    return np.concatenate([fn(params, *args, cts[s:s + step], luts, idx[s:s + step]) for s in range(0, len(cts), step)])


def _pbs_rows(job):
    params, terms, cts, luts, idx = job
    return pbs_exact_batch(params, terms, cts, luts, idx)


def pbs_exact_batch_parallel(params, terms, cts, luts, lut_idx, workers=12):
    """pbs_exact_batch with the rows spread over fresh numpy-only processes: real n times a hundred LWEs is a minute of
    single-threaded FFTs otherwise.  Small jobs run in place."""
    cts = np.asarray(cts, dtype=U64).reshape(-1, params.n + 1)
    idx = np.asarray(lut_idx, dtype=np.int64)
    if len(cts) * params.n < 20000:
        return pbs_exact_batch(params, terms, cts, luts, idx)
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    parts = [p for p in np.array_split(np.arange(len(cts)), workers) if len(p)]
    with ProcessPoolExecutor(len(parts), mp_context=multiprocessing.get_context("spawn")) as pool:
        return np.concatenate(list(pool.map(_pbs_rows, [(params, terms, cts[p], luts, idx[p]) for p in parts])))


# ---- f64 transform precision at full scale -----------------------------------------------------------------------------
#
# Under a uniformly random full-range key nothing is bit exact between two f64 implementations, but the per-coefficient
# error against the exact integers is a sample of the transform's rounding noise.  One external product per LWE (one
# non-zero mask word, or one multi-bit group) keeps every decomposition digit the same in both, so the error is that
# noise alone and an implementation's spread can be held against the oracle's f64 path.  The rig of
# tests/test_gpu_rotation_precision.py; tests/test_exact_pbs.py pins its bounds on the oracle itself.

ORACLE_ROWS = 16               # the reference spread comes from at most this many LWEs: the error's distribution is the same for every one


def twin(p, n, name=None):
    """The shape p with another small dimension n."""
    import dataclasses
    return dataclasses.replace(p, n=n, name=name or f"{p.name}_n{n}")


def signed_errors(got, want):
    """got - want on the u64 torus as signed f64, flat."""
    with np.errstate(over="ignore"):
        return (np.asarray(got, dtype=U64) - want).astype(np.int64).astype(np.float64).reshape(-1)


def one_cmux_inputs(p, rng, B):
    """Small-key LWEs with a random body and exactly one non-zero mask word: one CMUX each."""
    cts = np.zeros((B, p.n + 1), dtype=U64)
    cts[:, p.n] = rng.integers(0, 2**64, size=B, dtype=U64)
    pos = rng.integers(0, p.n, size=B)
    cts[np.arange(B), pos] = rng.integers(1, 2**64, size=B, dtype=U64)
    return cts


class PrecisionCase:
    """A full-range key, one table, `count` distinct LWEs of one external product each, their exact outputs, and the
    error of the oracle's f64 path on the first ORACLE_ROWS of them (e_orc [rows, big_size], s_orc its pooled std).
    grouping = 0: classic PBS, one_cmux_inputs; grouping = G: multi-bit on a shape with n = G, uniformly random LWEs."""

    def __init__(self, p, grouping, count, seed=0):
        import oracle as O
        assert not grouping or p.n == grouping
        self.p, self.G, self.count = p, grouping, count
        rng = np.random.default_rng([p.N, p.k, p.pbs_level, p.n, grouping, count, seed])
        n_ggsw = p.n // grouping * (1 << grouping) if grouping else p.n
        self.bsk = rng.integers(0, 2**64, size=(n_ggsw, p.pbs_level, p.k + 1, p.k + 1, p.N), dtype=U64)
        self.lut = rng.integers(0, 2**64, size=p.glwe_len, dtype=U64)
        terms = limb_terms(self.bsk)
        if grouping:
            self.cts = rng.integers(0, 2**64, size=(count, p.n + 1), dtype=U64)
            self.want = multi_bit_pbs_exact_batch(p, grouping, terms, self.cts, self.lut)
            sk = O.MultiBitServerKey.from_keys(p, grouping, self.bsk, threads=4)
        else:
            self.cts = self._live_one_cmux_inputs(p, rng, count)
            self.want = np.zeros((count, p.big_size), dtype=U64)
            pos = (self.cts[:, :p.n] != 0).argmax(axis=1)
            for i in np.unique(pos):                       # pbs_exact_batch skips a step no row of which is live: n times less work
                self.want[pos == i] = pbs_exact_batch(p, terms, self.cts[pos == i], self.lut)
            ksk = np.zeros(p.big_dim * p.ks_level * p.small_size, dtype=U64)
            sk = O.ServerKey.from_keys(p, self.bsk, ksk, threads=4)
        rows = min(count, ORACLE_ROWS)
        self.orc = np.stack([sk.pbs(c, self.lut) for c in self.cts[:rows]])
        self.e_orc = signed_errors(self.orc, self.want[:rows]).reshape(rows, -1)
        self.s_orc = self.e_orc.std()

    @staticmethod
    def _live_one_cmux_inputs(p, rng, count):
        """one_cmux_inputs whose mask word does not switch to X^0: there the CMUX multiplies by zero and the LWE would carry
        no error at all (one draw in 2N: one in 256 at N = 128)."""
        logN = p.N.bit_length() - 1
        while True:
            cts = one_cmux_inputs(p, rng, count)
            if all(modulus_switch(a, logN) % (2 * p.N) for a in cts[:, :p.n].max(axis=1)):
                return cts


def f64_precision_figures(errors, s_orc, distinct):
    """errors [slots, big_size]: an f64 implementation's signed error against exact on a PrecisionCase, slot by slot (slots
    beyond `distinct` repeat earlier inputs); s_orc: the oracle's spread on it.  Returns a dict of the figures the bounds read."""
    errors = np.asarray(errors, dtype=np.float64)
    m = errors.shape[1]
    s = errors.std()
    per_slot = errors.std(axis=1)
    # repeated slots repeat their values on a deterministic implementation: the mean has the spread of distinct * m samples
    n_eff = distinct * m
    return {"s": s, "s_orc": s_orc, "ratio": s / s_orc, "max": np.abs(errors).max(),
            "bias_sigmas": abs(errors.mean()) * np.sqrt(n_eff) / s if s else 0.0,
            "worst_slot": int(per_slot.argmax()), "worst_slot_ratio": per_slot.max() / s_orc,
            "slot_bound": 1.6 * (1 + 4 / np.sqrt(2 * m))}


def assert_f64_precision(name, errors, s_orc, distinct):
    """The three bounds an f64 blind rotation is held to, with one printed line of figures.
      * pooled: 0.25 s_orc < std <= 1.6 s_orc and max |e| < 8 s_orc -- its transforms are no noisier than the reference algorithm's;
      * per slot: the std over a slot's m = big_size coefficients <= 1.6 s_orc (1 + 4 / sqrt(2 m)): a std of m samples has
        relative sampling error 1 / sqrt(2 m), four of them allowed -- a loss on one of the workgroups sharing a CU, or on one
        round of a tiled batch, shows here and is diluted in the pool;
      * no bias: |mean| <= 5 std / sqrt(n) over the n independent coefficients -- a truncating from_torus or a dropped rounding."""
    f = f64_precision_figures(errors, s_orc, distinct)
    print(f"{name}: error std 2^{np.log2(f['s']):.2f}, oracle f64 2^{np.log2(s_orc):.2f} (ratio {f['ratio']:.3f}); max 2^{np.log2(f['max']):.2f} "
          f"({f['max'] / s_orc:.2f} s_orc); bias {f['bias_sigmas']:.2f} sigma/sqrt(n); worst slot {f['worst_slot']} of {len(errors)} at "
          f"{f['worst_slot_ratio']:.3f} s_orc (bound {f['slot_bound']:.3f})")
    assert 0.25 * s_orc < f["s"] <= 1.6 * s_orc
    assert f["max"] < 8 * s_orc
    assert f["worst_slot_ratio"] <= f["slot_bound"]
    assert f["bias_sigmas"] <= 5
    return f
