// ring_packing.h -- ring packing: big-key LWEs -> GLWEs through log2(N) automorphism keys (Chen, Dai, Kim, Song,
// "Efficient homomorphic conversion between (ring) LWE ciphertexts", 2021), the definition shared by the host reference
// (ring_packing.cpp) and the kernels (ring_packing_kernels.hip.h).  Includes standard headers, noise_model.h and
// include/fhestr.h only, so that the unit compiles stand-alone under a host sanitizer (tests/ring_packing_main.cpp).
//
// All ciphertext arithmetic is mod 2^64, wrapping; the phase is B - sum_q A_q S_q, the big LWE key the flattened GLWE key.
//   leaf      w' = (w + N/2) >> log2 N for every word of the LWE (the division that stands in for N^-1, which does not exist
//             mod 2^64); A_q[0] = a'[qN], A_q[i] = -a'[qN + N - i], B[0] = b', the rest 0.
//   autoKS_l  t = 2^l + 1, sigma_t(P)(X) = P(X^t): (0, .., 0, sigma_t(B)) - sum_q sum_it digit_it(sigma_t(A_q)) (*) AK[l][q][it],
//             the signed digits of the keyswitch (level L first: row `it` of a key polynomial belongs to level L - it) and
//             (*) the negacyclic product.
//   merge     node (l, r), r < s = N / 2^l, holds the leaves r, r + s, r + 2s, ..: e = node (l-1, r), o = node (l-1, r + s),
//             node (l, r) = (e + X^s o) + autoKS_l(e - X^s o).  Node (log2 N, 0) holds leaf j at coefficient j: the layout of
//             the packing keyswitch.  A node without a leaf is the zero ciphertext and costs nothing.
//   key       [log2 N][k][level, level L first][k+1][N] u64: AK[l][q][it] is a GLWE encryption of S_q(X^t) << (64 - b (L - it)).
//
// The products are exact.  A key polynomial is rewritten into eight balanced base-256 digit planes (ksk_repack_mfma_kernel's
// decomposition), every plane and every digit polynomial is transformed with a negacyclic number-theoretic transform mod
// RING_P, the pointwise products are summed over q and level, and the centred lift of the inverse transform is the integer
// sum as long as its magnitude k L N 2^(b-1) 128 stays below P / 2 (ring_packing_check).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/fhestr.h"

#if defined(__HIPCC__)
#define FHE_RING_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FHE_RING_HD inline
#endif

namespace fhe {

constexpr uint32_t RING_P = 4293918721u;          // 2^32 - 2^20 + 1, prime; 2^20 divides P - 1
constexpr uint32_t RING_N_MIN = 4, RING_N_MAX = 32768;   // one polynomial of 32-bit words in the LDS of one CU
constexpr uint32_t RING_PLANES = 8;

// x mod P for any 64-bit x, by 2^32 = 2^20 - 1 (mod P) three times: x < 2^64 -> < 2^52 + 2^32 -> < 2^40 + 2^32 -> < 2^28 + 2^32 < 2 P.
FHE_RING_HD uint32_t ring_reduce(uint64_t x) {
    x = ((x >> 32) << 20) - (x >> 32) + (uint32_t)x;
    x = ((x >> 32) << 20) - (x >> 32) + (uint32_t)x;
    x = ((x >> 32) << 20) - (x >> 32) + (uint32_t)x;
    return (uint32_t)(x >= RING_P ? x - RING_P : x);
}
FHE_RING_HD uint32_t ring_mul(uint32_t a, uint32_t b) { return ring_reduce((uint64_t)a * b); }
FHE_RING_HD uint32_t ring_add(uint32_t a, uint32_t b) {
    const uint64_t s = (uint64_t)a + b;
    return (uint32_t)(s >= RING_P ? s - RING_P : s);
}
FHE_RING_HD uint32_t ring_sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + (RING_P - b); }
FHE_RING_HD uint32_t ring_from_signed(int64_t v) { return v < 0 ? (uint32_t)((int64_t)RING_P + v) : (uint32_t)v; }   // |v| < P
FHE_RING_HD int64_t ring_lift(uint32_t v) { return v > RING_P / 2 ? (int64_t)v - (int64_t)RING_P : (int64_t)v; }   // centred

// Digit `it` (level L - it) of the closest representable value of x at b L bits: the keyswitch's signed decomposition
// (packing_decompose of client.cpp), |digit| <= 2^(b-1).
FHE_RING_HD int64_t ring_digit(uint64_t x, uint32_t bl, uint32_t L, uint32_t it) {
    const uint32_t rep = bl * L;
    const uint64_t mask = (1ull << bl) - 1;
    uint64_t state = (((x >> (63 - rep)) + 1) >> 1) & ((1ull << rep) - 1);
    int64_t digit = 0;
    for (uint32_t lv = 0; lv <= it; lv++) {
        const uint64_t res = state & mask;
        state >>= bl;
        const uint64_t carry = (((res - 1ull) | state) & res) >> (bl - 1);
        state += carry;
        digit = (int64_t)res - (int64_t)(carry << bl);
    }
    return digit;
}

// Balanced base-256 digit `plane` of a key word: w = sum_p digit_p 256^p (mod 2^64), every digit in [-128, 127].
FHE_RING_HD int32_t ring_plane(uint64_t w, uint32_t plane) {
    int8_t s = 0;
    for (uint32_t t = 0; t <= plane; t++) {
        s = (int8_t)(uint8_t)(w & 0xff);
        w = (w - (uint64_t)(int64_t)s) >> 8;
    }
    return s;
}

// Word of the leaf: the rounded division by N.
FHE_RING_HD uint64_t ring_leaf_word(uint64_t w, uint32_t logN) { return (w + ((1ull << logN) >> 1)) >> logN; }

// Coefficient c of sigma_t(P): +-P[j] with u = c t^-1 mod 2N, j = u mod N, negated when u >= N.  `tinv` is t^-1 mod 2N.
FHE_RING_HD uint32_t ring_auto_source(uint32_t N, uint32_t tinv, uint32_t c, bool* negate) {
    const uint32_t u = (c * tinv) & (2 * N - 1);
    *negate = u >= N;
    return u & (N - 1);
}
// Coefficient j of X^s o: o[j - s], or -o[j - s + N] below s.
FHE_RING_HD uint64_t ring_shifted(const uint64_t* o, uint32_t N, uint32_t s, uint32_t j) { return j >= s ? o[j - s] : 0 - o[j - s + N]; }

uint32_t ring_log2(uint32_t N);                   // N a power of two
uint32_t ring_tinv(uint32_t N, uint32_t level);   // (2^level + 1)^-1 mod 2N

// Twiddles of the negacyclic transform of size N: fwd[x] = psi^bitrev(x), inv[x] = psi^-bitrev(x) over log2 N bits, psi a
// primitive 2N-th root of unity mod P; n_inv = N^-1 mod P.
struct RingTables {
    uint32_t N = 0, n_inv = 0;
    std::vector<uint32_t> fwd, inv;
};
void ring_tables(uint32_t N, RingTables* out);
// In place, one polynomial of N residues below P.  Forward: natural order in, bit-reversed out; the inverse takes that back
// and multiplies by N^-1.
void ring_ntt_forward(const RingTables& t, uint32_t* a);
void ring_ntt_inverse(const RingTables& t, uint32_t* a);

// ---- parameters and model.  A std::string is empty, or the reason of the refusal. ----
std::string ring_packing_check(const fhe_params_t& p, const fhe_packing_params_t& pp);
uint64_t ring_packing_key_words(const fhe_params_t& p, const fhe_packing_params_t& pp);
// variance (torus = 1) ring packing adds to a packed coefficient: (N^2 / 3) V_aks + the division's term
double ring_packing_variance(const fhe_params_t& p, const fhe_packing_params_t& pp);
// log2 of the probability that a packed PBS output decodes wrongly at delta / 2, `extra` variance added; *target: the bound
double ring_packed_log2_pfail(const fhe_params_t& p, const fhe_packing_params_t& pp, double extra, double* target);
std::string ring_packing_default_params(const fhe_params_t& p, fhe_packing_params_t* out);
// out[0]: variance of a raw block extracted from a ring-packed PBS output, in nominal variances; out[1]: the PBS-input budget
void ring_packing_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, double out[2]);
// the same after narrowing to `bits`; out[2]: log2 of the client's decoding failure probability
void ring_narrow_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, uint32_t bits, double out[3]);
// automorphism keyswitches of packing `count` LWEs: sum over the GLWEs of sum_{d < log2 N} min(2^d, c)
uint64_t ring_pack_keyswitches(uint32_t N, uint32_t count);

// ---- the host reference ----
// sum over `terms` of a[t] (*) b[t], polynomials of N signed coefficients, through the transform: exact while the true
// magnitude stays below P / 2
void ring_product(const RingTables& t, uint32_t terms, const int32_t* a, const int32_t* b, int64_t* out);
// cts: count x (kN + 1) -> glwes: ceil(count / N) x [k+1][N]
std::string ring_pack(const fhe_params_t& p, const fhe_packing_params_t& pp, const uint64_t* key, const uint64_t* cts, uint32_t count, uint64_t* glwes);

}  // namespace fhe
