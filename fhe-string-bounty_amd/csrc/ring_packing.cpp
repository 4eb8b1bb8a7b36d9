// ring_packing.cpp -- ring packing on the host (ring_packing.h): the parameter check, the noise model, the negacyclic
// number-theoretic transform mod RING_P and the reference fhe_ring_pack_host, the plain definition with the transform as its
// exact product.  Standard headers only; no device code.
#include "ring_packing.h"

#include <math.h>
#include <string.h>

#include "noise_model.h"

namespace fhe {

uint32_t ring_log2(uint32_t N) {
    uint32_t l = 0;
    while ((1u << l) < N) l++;
    return l;
}

uint32_t ring_tinv(uint32_t N, uint32_t level) {
    const uint32_t m = 2 * N - 1, t = ((1u << level) + 1) & m;
    uint32_t x = 1;                                  // Newton: every step doubles the correct low bits of t^-1 mod 2^j
    for (int i = 0; i < 5; i++) x = (x * (2 - t * x)) & m;
    return x;
}

static uint32_t ring_pow(uint32_t b, uint64_t e) {
    uint32_t r = 1;
    for (; e; e >>= 1, b = ring_mul(b, b))
        if (e & 1) r = ring_mul(r, b);
    return r;
}

void ring_tables(uint32_t N, RingTables* out) {
    // a generator of the multiplicative group: P - 1 = 2^20 * 3^2 * 5 * 7 * 13
    uint32_t g = 2;
    for (;; g++) {
        bool ok = true;
        for (uint32_t r : {2u, 3u, 5u, 7u, 13u}) ok = ok && ring_pow(g, (RING_P - 1) / r) != 1;
        if (ok) break;
    }
    const uint32_t logN = ring_log2(N), psi = ring_pow(g, (RING_P - 1) / (2 * N)), psi_inv = ring_pow(psi, RING_P - 2);
    out->N = N;
    out->n_inv = ring_pow(N, RING_P - 2);
    out->fwd.assign(N, 0);
    out->inv.assign(N, 0);
    uint32_t f = 1, b = 1;
    for (uint32_t x = 0; x < N; x++) {               // power x lands at the bit-reversed index
        uint32_t rev = 0;
        for (uint32_t i = 0; i < logN; i++) rev |= ((x >> i) & 1) << (logN - 1 - i);
        out->fwd[rev] = f;
        out->inv[rev] = b;
        f = ring_mul(f, psi);
        b = ring_mul(b, psi_inv);
    }
}

void ring_ntt_forward(const RingTables& tb, uint32_t* a) {
    const uint32_t N = tb.N;
    uint32_t t = N;
    for (uint32_t m = 1; m < N; m <<= 1) {
        t >>= 1;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t S = tb.fwd[m + i];
            for (uint32_t j = 2 * i * t; j < 2 * i * t + t; j++) {
                const uint32_t U = a[j], V = ring_mul(a[j + t], S);
                a[j] = ring_add(U, V);
                a[j + t] = ring_sub(U, V);
            }
        }
    }
}

void ring_ntt_inverse(const RingTables& tb, uint32_t* a) {
    const uint32_t N = tb.N;
    uint32_t t = 1;
    for (uint32_t m = N; m > 1; m >>= 1, t <<= 1) {
        const uint32_t h = m >> 1;
        for (uint32_t i = 0; i < h; i++) {
            const uint32_t S = tb.inv[h + i];
            for (uint32_t j = 2 * i * t; j < 2 * i * t + t; j++) {
                const uint32_t U = a[j], V = a[j + t];
                a[j] = ring_add(U, V);
                a[j + t] = ring_mul(ring_sub(U, V), S);
            }
        }
    }
    for (uint32_t j = 0; j < N; j++) a[j] = ring_mul(a[j], tb.n_inv);
}

// ---- parameters and model -------------------------------------------------------------------------------------------------
uint64_t ring_packing_key_words(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    return (uint64_t)ring_log2(p.N) * p.k * pp.level * (p.k + 1) * p.N;
}

std::string ring_packing_check(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    if (p.k < 1 || p.k > 8 || p.N < RING_N_MIN || p.N > RING_N_MAX || (p.N & (p.N - 1)))
        return "ring packing: polynomial size must be a power of two in 4 .. 32768, k in 1 .. 8";
    if (pp.base_log < 1 || pp.base_log > 32 || pp.level < 1 || pp.level > 16 || pp.base_log * pp.level > 63)
        return "unsupported ring packing decomposition (base_log 1..32, level 1..16, base_log * level <= 63)";
    // largest magnitude of a sum over q and level of digit polynomial (*) plane: k L N 2^(b-1) 128, against the centred lift's P / 2
    const uint64_t bound = (uint64_t)p.k * pp.level * p.N * 128 << (pp.base_log - 1);
    if (bound >= RING_P / 2)
        return "ring packing: the pair (" + std::to_string(pp.base_log) + ", " + std::to_string(pp.level) + ") is over the one-prime bound: k L N 2^(b-1) 128 = " +
               std::to_string(bound) + " must stay below P / 2 = " + std::to_string(RING_P / 2);
    return "";
}

double ring_packing_variance(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    const double N = p.N, kN = (double)p.k * p.N, B = ldexp(1.0, (int)pp.base_log);
    const double v_aks = kN * pp.level * (B * B + 2) / 12.0 * p.glwe_std * p.glwe_std + kN / 2.0 / 12.0 * ldexp(1.0, -2 * (int)(pp.base_log * pp.level));
    return N * N / 3.0 * v_aks + N * N * kN / 24.0 * ldexp(1.0, -128);
}

// packed_log2_pfail of client.cpp with this route's variance: the bound a plan enforces at its PBS inputs
double ring_packed_log2_pfail(const fhe_params_t& p, const fhe_packing_params_t& pp, double extra, double* target) {
    const double max_level = (double)(p.msg_mod * p.carry_mod - 1) / (double)(p.msg_mod > 1 ? p.msg_mod - 1 : 1);
    NoiseModel m = noise_model(p);
    if (!noise_model_is_calibrated(p)) m.v_pbs *= kUncalibratedSafety;
    *target = m.log2_pfail(max_level * max_level) + (p.grouping_factor == 2 ? 0.0 : kPfailSlackLog2);
    NoiseModel packed = m;
    packed.v_ks = ring_packing_variance(p, pp) + extra;
    packed.v_ms = 0;
    return packed.log2_pfail(1.0);
}

std::string ring_packing_default_params(const fhe_params_t& p, fhe_packing_params_t* out) {
    out->base_log = out->level = 0;
    const std::string shape = ring_packing_check(p, fhe_packing_params_t{1, 1});
    if (!shape.empty()) return shape;                // (1, 1) is under the one-prime bound at every admitted shape
    for (uint32_t level = 1; level <= 16; level++)
        for (uint32_t base_log = 32; base_log >= 1; base_log--) {
            const fhe_packing_params_t pp{base_log, level};
            double target;
            if (!ring_packing_check(p, pp).empty() || ring_packed_log2_pfail(p, pp, 0.0, &target) > target) continue;
            *out = pp;
            return "";
        }
    return "ring packing: no decomposition under the one-prime bound meets the failure bound for this parameter set";
}

void ring_packing_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, double out[2]) {
    out[0] = 1.0 + ring_packing_variance(p, pp) / noise_model(p).v_pbs;
    out[1] = default_noise_budget(p);
}

void ring_narrow_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, uint32_t bits, double out[3]) {
    const double v_narrow = (1.0 + (double)p.k * p.N / 2.0) / 12.0 * ldexp(1.0, -2 * (int)bits);   // narrow_variance of client.cpp
    double unpack[2], target;
    ring_packing_noise(p, pp, unpack);
    out[0] = unpack[0] + v_narrow / noise_model(p).v_pbs;
    out[1] = unpack[1];
    out[2] = ring_packed_log2_pfail(p, pp, v_narrow, &target);
}

uint64_t ring_pack_keyswitches(uint32_t N, uint32_t count) {
    uint64_t total = 0;
    for (uint64_t at = 0; at < count; at += N) {
        const uint64_t c = count - at < N ? count - at : N;
        for (uint64_t s = 1; s < N; s <<= 1) total += s < c ? s : c;
    }
    return total;
}

// ---- the host reference ---------------------------------------------------------------------------------------------------
void ring_product(const RingTables& t, uint32_t terms, const int32_t* a, const int32_t* b, int64_t* out) {
    const uint32_t N = t.N;
    std::vector<uint32_t> fa(N), fb(N), acc(N, 0);
    for (uint32_t x = 0; x < terms; x++) {
        for (uint32_t i = 0; i < N; i++) {
            fa[i] = ring_from_signed(a[(size_t)x * N + i]);
            fb[i] = ring_from_signed(b[(size_t)x * N + i]);
        }
        ring_ntt_forward(t, fa.data());
        ring_ntt_forward(t, fb.data());
        for (uint32_t i = 0; i < N; i++) acc[i] = ring_add(acc[i], ring_mul(fa[i], fb[i]));
    }
    ring_ntt_inverse(t, acc.data());
    for (uint32_t i = 0; i < N; i++) out[i] = ring_lift(acc[i]);
}

std::string ring_pack(const fhe_params_t& p, const fhe_packing_params_t& pp, const uint64_t* key, const uint64_t* cts, uint32_t count, uint64_t* glwes) {
    const std::string why = ring_packing_check(p, pp);
    if (!why.empty()) return why;
    const uint32_t N = p.N, k = p.k, L = pp.level, logN = ring_log2(N), kL = k * L, k1 = k + 1;
    const size_t glwe_len = (size_t)k1 * N, big = (size_t)k * N + 1;
    if (!count) return "";
    RingTables tb;
    ring_tables(N, &tb);
    // the key's planes, transformed: [level of the tree][q L + it][k+1][plane][N]
    std::vector<uint32_t> planes((size_t)logN * kL * k1 * RING_PLANES * N);
    for (size_t row = 0; row < (size_t)logN * kL * k1; row++)
        for (uint32_t pl = 0; pl < RING_PLANES; pl++) {
            uint32_t* dst = planes.data() + (row * RING_PLANES + pl) * N;
            for (uint32_t i = 0; i < N; i++) dst[i] = ring_from_signed(ring_plane(key[row * N + i], pl));
            ring_ntt_forward(tb, dst);
        }
    // leaves: slot j is leaf j
    std::vector<uint64_t> slots((size_t)count * glwe_len, 0);
    for (uint32_t j = 0; j < count; j++) {
        const uint64_t* ct = cts + (size_t)j * big;
        uint64_t* leaf = slots.data() + (size_t)j * glwe_len;
        for (uint32_t q = 0; q < k; q++) {
            leaf[(size_t)q * N] = ring_leaf_word(ct[(size_t)q * N], logN);
            for (uint32_t i = 1; i < N; i++) leaf[(size_t)q * N + i] = 0 - ring_leaf_word(ct[(size_t)q * N + N - i], logN);
        }
        leaf[(size_t)k * N] = ring_leaf_word(ct[(size_t)k * N], logN);
    }
    std::vector<uint64_t> diff(N), sigma_b(N), prod(N);
    std::vector<uint32_t> digits((size_t)kL * N), acc(N);
    const std::vector<uint64_t> zero(glwe_len, 0);
    for (uint32_t level = 1; level <= logN; level++) {
        const uint32_t s = N >> level, tinv = ring_tinv(N, level);
        const uint32_t* lkey = planes.data() + (size_t)(level - 1) * kL * k1 * RING_PLANES * N;
        for (uint32_t at = 0; at < count; at += N) {
            const uint32_t c_g = count - at < N ? count - at : N;
            for (uint32_t r = 0; r < s && r < c_g; r++) {
                uint64_t* e = slots.data() + (size_t)(at + r) * glwe_len;
                const uint64_t* o = r + s < c_g ? slots.data() + (size_t)(at + r + s) * glwe_len : zero.data();
                for (uint32_t q = 0; q <= k; q++) {                 // sigma_t(e - X^s o), polynomial by polynomial
                    const uint64_t *eq = e + (size_t)q * N, *oq = o + (size_t)q * N;
                    for (uint32_t c = 0; c < N; c++) {
                        bool neg;
                        const uint32_t j = ring_auto_source(N, tinv, c, &neg);
                        const uint64_t v = eq[j] - ring_shifted(oq, N, s, j);
                        (q < k ? diff : sigma_b)[c] = neg ? 0 - v : v;
                    }
                    if (q == k) break;
                    for (uint32_t it = 0; it < L; it++) {
                        uint32_t* d = digits.data() + (size_t)(q * L + it) * N;
                        for (uint32_t c = 0; c < N; c++) d[c] = ring_from_signed(ring_digit(diff[c], pp.base_log, L, it));
                        ring_ntt_forward(tb, d);
                    }
                }
                for (uint32_t qo = 0; qo <= k; qo++) {
                    std::fill(prod.begin(), prod.end(), 0);
                    for (uint32_t pl = 0; pl < RING_PLANES; pl++) {
                        for (uint32_t i = 0; i < N; i++) {
                            uint64_t sum = 0;
                            for (uint32_t x = 0; x < kL; x++)
                                sum += ring_mul(digits[(size_t)x * N + i], lkey[(((size_t)x * k1 + qo) * RING_PLANES + pl) * N + i]);
                            acc[i] = ring_reduce(sum);
                        }
                        ring_ntt_inverse(tb, acc.data());
                        for (uint32_t c = 0; c < N; c++) prod[c] += (uint64_t)ring_lift(acc[c]) << (8 * pl);
                    }
                    uint64_t* eq = e + (size_t)qo * N;
                    const uint64_t* oq = o + (size_t)qo * N;
                    for (uint32_t c = 0; c < N; c++) eq[c] = eq[c] + ring_shifted(oq, N, s, c) - prod[c] + (qo == k ? sigma_b[c] : 0);
                }
            }
        }
    }
    for (uint32_t at = 0, g = 0; at < count; at += N, g++) memcpy(glwes + (size_t)g * glwe_len, slots.data() + (size_t)at * glwe_len, glwe_len * 8);
    return "";
}

}  // namespace fhe
