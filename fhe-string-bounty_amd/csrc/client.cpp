// client.cpp -- client side of the engine: secret keys, encryption, decryption, server-key
// generation.  CPU code by design: in the reference these are ClientKey operations that never run
// on the evaluation path (shortint/engine/client_side.rs:13-128, shortint/client_key/mod.rs:281-337,
// shortint/engine/server_side.rs:54-160) and SURVEY.md section 8(f) ranks device-side key generation
// as a later row.  Randomness: ChaCha20 keystream under a 256-bit seed, one stream per purpose and key
// row (det_math.h; stands in for the reference's AES-128-CTR concrete-csprng with forked generators);
// noise follows the reference's Gaussian sampler
// (core_crypto/commons/math/random/gaussian.rs:17-47, polar method on two signed 64-bit draws) --
// both live in det_math.h, shared with the device-side key generation kernels.
#include <errno.h>
#include <sys/random.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "cast.h"
#include "det_math.h"
#include "engine.h"
#include "glwe_narrow.h"
#include "noise_model.h"
#include "ring_packing.h"

namespace fhe {

struct ClientKey {
    fhe_params_t p;
    Seed256 seed;
    std::vector<uint64_t> glwe_sk;    // k*N bits; also the big LWE key (client_side.rs:29)
    std::vector<uint64_t> small_sk;   // n bits
    Rng enc_rng;

    ClientKey(const fhe_params_t& params, const Seed256& seed_)
        : p(params), seed(seed_), glwe_sk((size_t)params.k * params.N), small_sk(params.n), enc_rng(seed_, 3) {
        fill_binary(glwe_sk, 1);
        fill_binary(small_sk, 2);
    }
    void fill_binary(std::vector<uint64_t>& key, uint64_t stream) {   // client_side.rs:13-27
        Rng r(seed, stream);
        for (size_t i = 0; i < key.size(); i += 64) {
            const uint64_t w = r.next();
            for (size_t b = 0; b < 64 && i + b < key.size(); b++) key[i + b] = (w >> b) & 1;
        }
    }
    uint64_t delta() const { return (1ull << 63) / ((uint64_t)p.msg_mod * p.carry_mod); }

    // core_crypto/algorithms/lwe_encryption.rs:61-110
    static void lwe_encrypt(const uint64_t* sk, size_t dim, uint64_t pt, double std_dev, Rng& r, uint64_t* ct) {
        uint64_t acc = 0;
        for (size_t i = 0; i < dim; i++) {
            ct[i] = r.next();
            acc += ct[i] * sk[i];
        }
        ct[dim] = acc + gaussian_torus(r, std_dev) + pt;
    }
    uint64_t phase(const uint64_t* ct) const {
        const size_t dim = glwe_sk.size();
        uint64_t acc = 0;
        for (size_t i = 0; i < dim; i++) acc += ct[i] * glwe_sk[i];
        return ct[dim] - acc;
    }
    // shortint/client_key/mod.rs:281-303
    uint64_t decode(uint64_t x) const {
        const uint64_t d = delta(), rounding = (x & (d >> 1)) << 1;
        return (x + rounding) / d;
    }

    // lwe_keyswitch_key_generation.rs:65-130, for any pair of LWE keys: row (i, it) encrypts in_sk[i] at level `level - it`
    // under out_sk; one generator per input key bit.  The clients' own keyswitch key and the casting keys (cast.h).
    static void gen_lwe_ksk(const uint64_t* in_sk, size_t in_dim, const uint64_t* out_sk, size_t out_dim, uint32_t base_log, uint32_t level,
                            double std_dev, const Seed256& seed, uint64_t stream_base, uint64_t* ksk) {
        for (size_t i = 0; i < in_dim; i++) {
            Rng r(seed, stream_base + i);
            for (uint32_t it = 0; it < level; it++) {
                const uint64_t pt = in_sk[i] << (64 - base_log * (level - it));
                lwe_encrypt(out_sk, out_dim, pt, std_dev, r, ksk + (i * level + it) * (out_dim + 1));
            }
        }
    }
    void gen_ksk(uint64_t* ksk) const {
        gen_lwe_ksk(glwe_sk.data(), glwe_sk.size(), small_sk.data(), p.n, p.ks_base_log, p.ks_level, p.lwe_std, seed, 0x4B534B0000000000ull, ksk);
    }
    // glwe_encryption.rs:17-60 with a binary key: body += e + sum_q A_q * S_q (signed shifts)
    void glwe_encrypt_assign(uint64_t* glwe, Rng& r) const {
        const uint32_t N = p.N, k = p.k;
        uint64_t* body = glwe + (size_t)k * N;
        for (size_t j = 0; j < (size_t)k * N; j++) glwe[j] = r.next();
        for (uint32_t j = 0; j < N; j++) body[j] += gaussian_torus(r, p.glwe_std);
        for (uint32_t q = 0; q < k; q++) {
            const uint64_t *a = glwe + (size_t)q * N, *s = glwe_sk.data() + (size_t)q * N;
            for (uint32_t t = 0; t < N; t++) {
                if (!s[t]) continue;
                for (uint32_t c = 0; c < N - t; c++) body[c + t] += a[c];
                for (uint32_t c = N - t; c < N; c++) body[c + t - N] -= a[c];
            }
        }
    }
    // lwe_bootstrap_key_generation.rs:76-135 + ggsw_encryption.rs:72-151,300-331
    // plaintext bit of every GGSW of the key (classic: the small key; multi-bit: per-group products)
    std::vector<uint64_t> ggsw_bits() const {
        const uint32_t ng = n_ggsw(p), gf = p.grouping_factor > 1 ? p.grouping_factor : 1;
        std::vector<uint64_t> bits(ng);
        for (uint32_t i = 0; i < ng; i++)
            bits[i] = gf == 1 ? small_sk[i]
                              : multi_bit_key_bit(small_sk.data() + (size_t)(i >> gf) * gf, gf, i & ((1u << gf) - 1));
        return bits;
    }
    // (multi-bit: lwe_multi_bit_bootstrap_key_generation.rs:87-173, the same GGSW encryption per entry)
    void gen_bsk_range(uint64_t* bsk, const uint64_t* bits, size_t lo, size_t hi) const {
        const uint32_t N = p.N, k = p.k, k1 = k + 1, L = p.pbs_level;
        const size_t glwe_len = (size_t)k1 * N, ggsw_len = (size_t)L * k1 * glwe_len;
        for (size_t i = lo; i < hi; i++) {
            Rng r(seed, 0x42534B0000000000ull + i);
            uint64_t* ggsw = bsk + i * ggsw_len;
            const uint64_t m = bits[i];
            for (uint32_t li = 0; li < L; li++) {
                const uint64_t factor = (0 - m) * (1ull << (64 - p.pbs_base_log * (li + 1)));
                for (uint32_t row = 0; row < k1; row++) {
                    uint64_t* glwe = ggsw + ((size_t)li * k1 + row) * glwe_len;
                    uint64_t* body = glwe + (size_t)k * N;
                    if (row < k) {
                        const uint64_t* s = glwe_sk.data() + (size_t)row * N;
                        for (uint32_t c = 0; c < N; c++) body[c] = s[c] * factor;
                    } else {
                        std::memset(body, 0, N * sizeof(uint64_t));
                        body[0] = 0 - factor;
                    }
                    glwe_encrypt_assign(glwe, r);
                }
            }
        }
    }
    // lwe_packing_keyswitch_key_generation.rs:19-96: key bit i, level l -> GLWE encryption of the constant s_i << (64 - base_log l)
    void gen_packing_key_range(const fhe_packing_params_t& pp, const Seed256& key_seed, uint64_t* pksk, size_t lo, size_t hi) const {
        const size_t glwe_len = (size_t)(p.k + 1) * p.N;
        for (size_t i = lo; i < hi; i++) {
            Rng r(key_seed, 0x504B534B00000000ull + i);
            for (uint32_t it = 0; it < pp.level; it++) {
                const uint32_t level = pp.level - it;
                uint64_t* glwe = pksk + (i * pp.level + it) * glwe_len;
                uint64_t* body = glwe + (size_t)p.k * p.N;
                std::memset(body, 0, p.N * sizeof(uint64_t));
                body[0] = glwe_sk[i] << (64 - pp.base_log * level);
                glwe_encrypt_assign(glwe, r);
            }
        }
    }
    // ring_packing.h: tree level l, key polynomial q, level row `it` -> GLWE encryption of S_q(X^t) << (64 - base_log (L - it)), t = 2^l + 1
    void gen_ring_packing_key_range(const fhe_packing_params_t& pp, const Seed256& key_seed, uint64_t* key, size_t lo, size_t hi) const {
        const uint32_t N = p.N;
        const size_t glwe_len = (size_t)(p.k + 1) * N;
        for (size_t row = lo; row < hi; row++) {            // row = (l - 1) k + q
            const uint32_t level = (uint32_t)(row / p.k) + 1, q = (uint32_t)(row % p.k), tinv = ring_tinv(N, level);
            Rng r(key_seed, 0x52504B0000000000ull + row);
            for (uint32_t it = 0; it < pp.level; it++) {
                uint64_t* glwe = key + (row * pp.level + it) * glwe_len;
                uint64_t* body = glwe + (size_t)p.k * N;
                const uint32_t shift = 64 - pp.base_log * (pp.level - it);
                for (uint32_t c = 0; c < N; c++) {
                    bool neg;
                    const uint64_t bit = glwe_sk[(size_t)q * N + ring_auto_source(N, tinv, c, &neg)];
                    body[c] = (neg ? 0 - bit : bit) << shift;
                }
                glwe_encrypt_assign(glwe, r);
            }
        }
    }
    // glwe_encryption.rs:438-470 (decrypt_glwe_ciphertext): body - sum_q A_q S_q, by shifted adds for the binary key
    void glwe_phase(const uint64_t* glwe, uint64_t* out) const {
        const uint32_t N = p.N, k = p.k;
        std::memcpy(out, glwe + (size_t)k * N, N * sizeof(uint64_t));
        for (uint32_t q = 0; q < k; q++) {
            const uint64_t *a = glwe + (size_t)q * N, *s = glwe_sk.data() + (size_t)q * N;
            for (uint32_t t = 0; t < N; t++) {
                if (!s[t]) continue;
                for (uint32_t c = 0; c < N - t; c++) out[c + t] -= a[c];
                for (uint32_t c = N - t; c < N; c++) out[c + t - N] += a[c];
            }
        }
    }
    void gen_bsk(uint64_t* bsk, int threads) const {
        if (threads < 1) threads = 1;
        const std::vector<uint64_t> bits = ggsw_bits();
        const size_t ng = bits.size();
        const uint64_t* b = bits.data();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([=] { gen_bsk_range(bsk, b, ng * t / threads, ng * (t + 1) / threads); });
        for (auto& th : pool) th.join();
    }
};

// ---- packing keyswitch (lwe_packing_keyswitch.rs): parameter checks, default decomposition, the plain host loop ----
constexpr uint64_t kPackingKeyMaxBytes = 1ull << 32;

static uint64_t packing_key_words(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    return (uint64_t)p.k * p.N * pp.level * (p.k + 1) * p.N;
}

int packing_params_check(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    if (p.k < 1 || p.N < 32 || (p.N & (p.N - 1))) return fail("packing keyswitch: polynomial size must be a power of two >= 32");
    if (pp.base_log < 1 || pp.base_log > 7 || pp.level < 1 || pp.level > 16 || pp.base_log * pp.level > 63)
        return fail("unsupported packing decomposition (base_log 1..7, level 1..16, base_log * level <= 63)");
    if (packing_key_words(p, pp) * 8 > kPackingKeyMaxBytes)
        return fail("unsupported parameter set for the packing keyswitch: the key would hold " +
                    std::to_string(packing_key_words(p, pp) * 8) + " bytes (limit 4 GiB)");
    return 0;
}

// Variance (torus = 1) the packing adds to a coefficient of a full GLWE.  Every one of the N packed LWEs brings one noise
// coefficient of each of its k N level key encryptions to EVERY coefficient (the rotation only moves them), so the key term
// of NoiseModel::v_ks counts N times, with the GLWE noise; the rounding of the mask against the binary key is the
// coefficient's own LWE's alone.
static double packing_variance(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    const double kN = (double)p.k * p.N, B = ldexp(1.0, (int)pp.base_log);
    return (double)p.N * kN * pp.level * (B * B + 2) / 12.0 * p.glwe_std * p.glwe_std +
           kN / 2.0 / 12.0 * ldexp(1.0, -2 * (int)(pp.base_log * pp.level));
}

// The bound a plan enforces at every PBS input (default_noise_budget): the failure probability of the reference-shaped
// worst case, with the same slack and the same safety on shapes whose V_pbs is unmeasured.  A packed coefficient is a PBS
// output (one nominal variance) plus the packing's own terms, decoded at delta / 2.
// `extra`: variance added to the coefficient after the packing (the narrowing's, narrow_noise).
// Returns log2 of the coefficient's decoding failure probability; *target receives the bound.
static double packed_log2_pfail(const fhe_params_t& p, const fhe_packing_params_t& pp, double extra, double* target) {
    const double max_level = (double)(p.msg_mod * p.carry_mod - 1) / (double)(p.msg_mod > 1 ? p.msg_mod - 1 : 1);
    NoiseModel m = noise_model(p);
    if (!noise_model_is_calibrated(p)) m.v_pbs *= kUncalibratedSafety;
    *target = m.log2_pfail(max_level * max_level) + (p.grouping_factor == 2 ? 0.0 : kPfailSlackLog2);
    NoiseModel packed = m;
    packed.v_ks = packing_variance(p, pp) + extra;
    packed.v_ms = 0;
    return packed.log2_pfail(1.0);
}

static bool packing_meets_bound(const fhe_params_t& p, const fhe_packing_params_t& pp) {
    double target;
    return packed_log2_pfail(p, pp, 0.0, &target) <= target;
}

// A packed PBS output extracted again (glwe_extract_kernels.hip.h moves words, it adds nothing): the PBS output's one
// nominal variance plus the packing keyswitch's, in units of V_pbs -- what a plan would have to declare for such an input.
// out[1]: the budget a plan enforces at its PBS inputs, which the refreshing PBS of fhe_engine_unpack_glwes must meet.
void packing_unpack_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, double out[2]) {
    out[0] = 1.0 + packing_variance(p, pp) / noise_model(p).v_pbs;
    out[1] = default_noise_budget(p);
}

// Narrowing to b bits (glwe_narrow.h) rounds every word of the GLWE to a multiple of 2^-b: an extracted block's phase
// gathers the body's rounding error and, through the binary key, about k N / 2 of the mask's -- the average-case form of
// v_ms and v_pbs_round, uniform errors of variance 2^-2b / 12 each.
static double narrow_variance(const fhe_params_t& p, uint32_t bits) {
    return (1.0 + (double)p.k * p.N / 2.0) / 12.0 * ldexp(1.0, -2 * (int)bits);
}

void narrow_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, uint32_t bits, double out[3]) {
    double unpack[2], target;
    packing_unpack_noise(p, pp, unpack);
    out[0] = unpack[0] + narrow_variance(p, bits) / noise_model(p).v_pbs;
    out[1] = unpack[1];
    out[2] = packed_log2_pfail(p, pp, narrow_variance(p, bits), &target);
}

// glwe_sample_extraction.rs:91-147 at coefficient c: the mask of polynomial q reversed from c downwards, the wrapped part
// negated; the body is B[c]
static void glwe_sample_extract_host(const fhe_params_t& p, const uint64_t* glwes, uint32_t first, uint32_t count, uint64_t* cts) {
    const uint32_t N = p.N, k = p.k;
    const size_t glwe_len = (size_t)(k + 1) * N, big = (size_t)k * N + 1;
    for (uint32_t r = 0; r < count; r++) {
        const uint64_t block = (uint64_t)first + r;
        const uint32_t c = (uint32_t)(block % N);
        const uint64_t* glwe = glwes + (size_t)(block / N) * glwe_len;
        uint64_t* ct = cts + (size_t)r * big;
        for (uint32_t q = 0; q < k; q++) {
            const uint64_t* a = glwe + (size_t)q * N;
            uint64_t* o = ct + (size_t)q * N;
            for (uint32_t i = 0; i <= c; i++) o[i] = a[c - i];
            for (uint32_t i = c + 1; i < N; i++) o[i] = 0 - a[N + c - i];
        }
        ct[(size_t)k * N] = glwe[(size_t)k * N + c];
    }
}

static inline void packing_decompose(uint64_t x, uint32_t bl, uint32_t L, int64_t* digits) {   // level L first (iter.rs:101-127)
    const uint32_t rep = bl * L;
    const uint64_t mask = (1ull << bl) - 1;
    uint64_t state = (((x >> (63 - rep)) + 1) >> 1) & ((1ull << rep) - 1);
    for (uint32_t lv = 0; lv < L; lv++) {
        uint64_t res = state & mask;
        state >>= bl;
        uint64_t carry = (((res - 1ull) | state) & res) >> (bl - 1);
        state += carry;
        digits[lv] = (int64_t)res - (int64_t)(carry << bl);
    }
}

static void packing_keyswitch_host(const fhe_params_t& p, const fhe_packing_params_t& pp, const uint64_t* pksk, const uint64_t* cts,
                                   uint32_t count, uint64_t* glwes) {
    const uint32_t N = p.N;
    const size_t in_dim = (size_t)p.k * N, glwe_len = (size_t)(p.k + 1) * N;
    std::memset(glwes, 0, (size_t)((count + N - 1) / N) * glwe_len * 8);
    std::vector<uint64_t> t(glwe_len);
    int64_t digits[16];
    for (uint32_t j = 0; j < count; j++) {
        const uint64_t* ct = cts + (size_t)j * (in_dim + 1);
        std::fill(t.begin(), t.end(), 0);
        t[(size_t)p.k * N] = ct[in_dim];
        for (size_t i = 0; i < in_dim; i++) {
            packing_decompose(ct[i], pp.base_log, pp.level, digits);
            for (uint32_t lv = 0; lv < pp.level; lv++) {
                if (!digits[lv]) continue;
                const uint64_t d = (uint64_t)digits[lv], *row = pksk + (i * pp.level + lv) * glwe_len;
                for (size_t c = 0; c < glwe_len; c++) t[c] -= d * row[c];
            }
        }
        uint64_t* out = glwes + (size_t)(j / N) * glwe_len;
        const uint32_t d = j % N;                                              // times X^d in Z[X] / (X^N + 1)
        for (uint32_t q = 0; q <= p.k; q++) {
            uint64_t* o = out + (size_t)q * N;
            const uint64_t* src = t.data() + (size_t)q * N;
            for (uint32_t c = 0; c < N - d; c++) o[c + d] += src[c];
            for (uint32_t c = N - d; c < N; c++) o[c + d - N] -= src[c];
        }
    }
}

}  // namespace fhe

struct fhe_client_key {
    fhe::ClientKey* impl;
};

extern "C" {

size_t fhe_params_ksk_len(const fhe_params_t* p) { return (size_t)p->k * p->N * p->ks_level * (p->n + 1); }
size_t fhe_params_bsk_len(const fhe_params_t* p) {
    return (size_t)fhe::n_ggsw(*p) * p->pbs_level * (p->k + 1) * (p->k + 1) * p->N;
}

int fhe_random_seed(uint8_t seed[32]) {
    if (!seed) return fhe::fail("null pointer: seed");
    size_t got = 0;
    while (got < 32) {                       // the kernel's CSPRNG (getrandom(2)); never blocks once initialised
        const ssize_t r = getrandom(seed + got, 32 - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return fhe::fail("getrandom failed: no entropy source");
        }
        got += (size_t)r;
    }
    return 0;
}

int fhe_chacha20_block(const uint8_t key[32], uint64_t counter, uint64_t stream, uint32_t out[16]) {
    if (!key || !out) return fhe::fail("null pointer");
    fhe::chacha20_block(fhe::seed_from_bytes(key), counter, stream, out);
    return 0;
}

int fhe_client_key_create(const fhe_params_t* params, const uint8_t seed[32], fhe_client_key** out) {
    if (!out) return fhe::fail("null pointer: out");
    *out = nullptr;
    if (!params) return fhe::fail("null pointer: params");
    if (!seed) return fhe::fail("null pointer: seed");
    try {
        *out = new fhe_client_key{new fhe::ClientKey(*params, fhe::seed_from_bytes(seed))};
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_client_key_destroy(fhe_client_key* ck) {
    if (ck) {
        delete ck->impl;
        delete ck;
    }
    return 0;
}

int fhe_client_encrypt(fhe_client_key* ck, const uint64_t* msgs, uint32_t count, uint64_t* cts) {
    if (!ck || !msgs || !cts) return fhe::fail("null pointer");
    auto& c = *ck->impl;
    const size_t dim = c.glwe_sk.size();
    for (uint32_t i = 0; i < count; i++)
        fhe::ClientKey::lwe_encrypt(c.glwe_sk.data(), dim, msgs[i] * c.delta(), c.p.glwe_std, c.enc_rng,
                                    cts + (size_t)i * (dim + 1));
    return 0;
}

int fhe_client_decrypt(fhe_client_key* ck, const uint64_t* cts, uint32_t count, uint64_t* msgs) {
    if (!ck || !msgs || !cts) return fhe::fail("null pointer");
    auto& c = *ck->impl;
    const size_t dim = c.glwe_sk.size();
    for (uint32_t i = 0; i < count; i++) msgs[i] = c.decode(c.phase(cts + (size_t)i * (dim + 1)));
    return 0;
}

int fhe_client_gen_server_keys(fhe_client_key* ck, uint64_t* bsk_std, uint64_t* ksk, int threads) {
    if (!ck || !bsk_std || !ksk) return fhe::fail("null pointer");
    try {
        ck->impl->gen_ksk(ksk);
        ck->impl->gen_bsk(bsk_std, threads);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_client_gen_compact_public_key(fhe_client_key* ck, const uint8_t seed[32], uint64_t* pk_out) {
    if (!ck || !seed || !pk_out) return fhe::fail("null pointer");
    try {
        auto& c = *ck->impl;
        const int threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        return fhe::compact_pk_generate(c.p, c.glwe_sk.data(), fhe::seed_from_bytes(seed), pk_out, threads);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
}

int fhe_packing_default_params(const fhe_params_t* params, fhe_packing_params_t* out) {
    if (!params || !out) return fhe::fail("null pointer");
    out->base_log = out->level = 0;
    for (uint32_t level = 1; level <= 16; level++)
        for (uint32_t base_log = 7; base_log >= 1; base_log--) {
            const fhe_packing_params_t pp{base_log, level};
            if (base_log * level > 63 || !fhe::packing_meets_bound(*params, pp)) continue;
            if (fhe::packing_params_check(*params, pp)) return 1;       // the cheapest pair that decrypts is already too large
            *out = pp;
            return 0;
        }
    return fhe::fail("packing keyswitch: no decomposition meets the failure bound for this parameter set");
}

size_t fhe_packing_key_len(const fhe_params_t* params, const fhe_packing_params_t* pp) {
    if (!params || !pp || fhe::packing_params_check(*params, *pp)) return 0;
    return (size_t)fhe::packing_key_words(*params, *pp);
}

size_t fhe_packed_glwe_len(const fhe_params_t* params, uint32_t count) {
    if (!params || !params->N) return 0;
    return (size_t)((count + params->N - 1) / params->N) * (params->k + 1) * params->N;
}

int fhe_client_gen_packing_key(fhe_client_key* ck, const fhe_packing_params_t* pp, const uint8_t seed[32], uint64_t* pksk_out,
                               int threads) {
    if (!ck || !pp || !seed || !pksk_out) return fhe::fail("null pointer");
    try {
        const auto& c = *ck->impl;
        if (fhe::packing_params_check(c.p, *pp)) return 1;
        threads = std::max(1, std::min(threads, 64));
        const fhe::Seed256 key_seed = fhe::seed_from_bytes(seed);
        const fhe_packing_params_t dec = *pp;
        const size_t rows = c.glwe_sk.size();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] { c.gen_packing_key_range(dec, key_seed, pksk_out, rows * t / threads, rows * (t + 1) / threads); });
        for (auto& th : pool) th.join();
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_client_decrypt_packed(fhe_client_key* ck, const uint64_t* glwes, uint32_t count, uint64_t* msgs) {
    if (!ck || (count && (!glwes || !msgs))) return fhe::fail("null pointer");
    try {
        const auto& c = *ck->impl;
        const uint32_t N = c.p.N;
        const size_t glwe_len = (size_t)(c.p.k + 1) * N;
        std::vector<uint64_t> ph(N);
        for (uint32_t g = 0; g * N < count; g++) {
            c.glwe_phase(glwes + (size_t)g * glwe_len, ph.data());
            for (uint32_t j = g * N; j < count && j < (g + 1) * N; j++) msgs[j] = c.decode(ph[j - g * N]);
        }
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_packing_keyswitch_host(const fhe_params_t* params, const fhe_packing_params_t* pp, const uint64_t* pksk, const uint64_t* cts,
                               uint32_t count, uint64_t* glwes) {
    if (!params || !pp || !pksk || !glwes || (count && !cts)) return fhe::fail("null pointer");
    try {
        if (fhe::packing_params_check(*params, *pp)) return 1;
        fhe::packing_keyswitch_host(*params, *pp, pksk, cts, count, glwes);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_glwe_sample_extract_host(const fhe_params_t* params, const uint64_t* glwes, uint32_t first, uint32_t count, uint64_t* cts) {
    if (!params || (count && (!glwes || !cts))) return fhe::fail("null pointer");
    if (params->k < 1 || params->N < 1) return fhe::fail("glwe sample extraction: k >= 1 and N >= 1");
    try {
        fhe::glwe_sample_extract_host(*params, glwes, first, count, cts);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_packing_unpack_noise(const fhe_params_t* params, const fhe_packing_params_t* pp, double out[2]) {
    if (!params || !pp || !out) return fhe::fail("null pointer");
    out[0] = out[1] = 0;
    if (fhe::packing_params_check(*params, *pp)) return 1;
    fhe::packing_unpack_noise(*params, *pp, out);
    return 0;
}

// ---- casting keys (cast.h, cast.cpp) ------------------------------------------------------------------------------------
static int cast_answer(const std::string& why) { return why.empty() ? 0 : fhe::fail(why); }

int fhe_cast_default_params(const fhe_params_t* src, const fhe_params_t* dst, uint32_t target, fhe_cast_params_t* cp) {
    if (!src || !dst || !cp) return fhe::fail("null pointer");
    return cast_answer(fhe::cast_default_params(*src, *dst, target, cp));
}

size_t fhe_cast_key_len(const fhe_params_t* dst, const fhe_cast_params_t* cp) {
    if (!dst || !cp || cast_answer(fhe::cast_params_check(*dst, *cp))) return 0;
    return (size_t)fhe::cast_key_words(*dst, *cp);
}

int fhe_cast_rshift(const fhe_params_t* src, const fhe_params_t* dst, int32_t* shift) {
    if (!src || !dst || !shift) return fhe::fail("null pointer");
    *shift = 0;
    return cast_answer(fhe::cast_rshift(*src, *dst, shift));
}

int fhe_cast_regroup_check(const fhe_params_t* src, const fhe_params_t* dst, uint32_t group, uint64_t* degree, uint64_t* space) {
    if (!src || !dst || !degree || !space) return fhe::fail("null pointer");
    *degree = *space = 0;
    return cast_answer(fhe::cast_regroup_check(*src, *dst, group, degree, space));
}

int fhe_client_gen_cast_key(fhe_client_key* ck_src, fhe_client_key* ck_dst, const fhe_cast_params_t* cp, const uint8_t seed[32], uint64_t* out) {
    if (!ck_src || !ck_dst || !cp || !seed || !out) return fhe::fail("null pointer");
    try {
        const auto &s = *ck_src->impl, &d = *ck_dst->impl;
        if (cast_answer(fhe::cast_params_check(d.p, *cp))) return 1;
        if (s.p.k != cp->src.k || s.p.N != cp->src.N) return fhe::fail("casting key: the source client key is not of the source parameter set");
        const bool small = cp->target == FHE_CAST_TO_SMALL;
        fhe::ClientKey::gen_lwe_ksk(s.glwe_sk.data(), s.glwe_sk.size(), small ? d.small_sk.data() : d.glwe_sk.data(), fhe::cast_out_dim(d.p, *cp), cp->base_log,
                                    cp->level, d.p.lwe_std, fhe::seed_from_bytes(seed), 0x43534B0000000000ull, out);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_cast_host(const fhe_params_t* dst, const fhe_cast_params_t* cp, const uint64_t* key, const uint64_t* in, uint32_t count, uint64_t* out) {
    if (!dst || !cp || !key || (count && (!in || !out))) return fhe::fail("null pointer");
    try {
        if (cast_answer(fhe::cast_params_check(*dst, *cp))) return 1;
        fhe::cast_keyswitch_host(*dst, *cp, key, in, count, out);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_cast_noise(const fhe_params_t* dst, const fhe_cast_params_t* cp, double v_in, double out[3]) {
    if (!dst || !cp || !out) return fhe::fail("null pointer");
    out[0] = out[1] = out[2] = 0;
    if (cast_answer(fhe::cast_params_check(*dst, *cp))) return 1;
    fhe::cast_noise(*dst, *cp, v_in, out);
    return 0;
}

// ---- ring packing (ring_packing.h) ----
static int ring_answer(const std::string& why) { return why.empty() ? 0 : fhe::fail(why); }

int fhe_ring_packing_default_params(const fhe_params_t* params, fhe_packing_params_t* out) {
    if (!params || !out) return fhe::fail("null pointer");
    return ring_answer(fhe::ring_packing_default_params(*params, out));
}

size_t fhe_ring_packing_key_len(const fhe_params_t* params, const fhe_packing_params_t* pp) {
    if (!params || !pp || ring_answer(fhe::ring_packing_check(*params, *pp))) return 0;
    return (size_t)fhe::ring_packing_key_words(*params, *pp);
}

int fhe_ring_packing_noise(const fhe_params_t* params, const fhe_packing_params_t* pp, double out[2]) {
    if (!params || !pp || !out) return fhe::fail("null pointer");
    out[0] = out[1] = 0;
    if (ring_answer(fhe::ring_packing_check(*params, *pp))) return 1;
    fhe::ring_packing_noise(*params, *pp, out);
    return 0;
}

int fhe_ring_narrow_noise(const fhe_params_t* params, const fhe_packing_params_t* pp, uint32_t bits, double out[3]) {
    if (!params || !pp || !out) return fhe::fail("null pointer");
    out[0] = out[1] = out[2] = 0;
    if (!fhe::narrow_bits_ok(bits)) return fhe::fail("narrow: the width must be 8 .. 32 bits");
    if (ring_answer(fhe::ring_packing_check(*params, *pp))) return 1;
    fhe::ring_narrow_noise(*params, *pp, bits, out);
    return 0;
}

uint64_t fhe_ring_pack_keyswitches(const fhe_params_t* params, uint32_t count) {
    return params && params->N ? fhe::ring_pack_keyswitches(params->N, count) : 0;
}

int fhe_client_gen_ring_packing_key(fhe_client_key* ck, const fhe_packing_params_t* pp, const uint8_t seed[32], uint64_t* key_out, int threads) {
    if (!ck || !pp || !seed || !key_out) return fhe::fail("null pointer");
    try {
        const auto& c = *ck->impl;
        if (ring_answer(fhe::ring_packing_check(c.p, *pp))) return 1;
        const fhe::Seed256 key_seed = fhe::seed_from_bytes(seed);
        const fhe_packing_params_t dec = *pp;
        const size_t rows = (size_t)fhe::ring_log2(c.p.N) * c.p.k;
        threads = (int)std::max<size_t>(1, std::min<size_t>(std::min(threads, 64), rows));
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] { c.gen_ring_packing_key_range(dec, key_seed, key_out, rows * t / threads, rows * (t + 1) / threads); });
        for (auto& th : pool) th.join();
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_ring_pack_host(const fhe_params_t* params, const fhe_packing_params_t* pp, const uint64_t* key, const uint64_t* cts, uint32_t count,
                       uint64_t* glwes) {
    if (!params || !pp || !key || (count && (!cts || !glwes))) return fhe::fail("null pointer");
    try {
        return ring_answer(fhe::ring_pack(*params, *pp, key, cts, count, glwes));
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
}

static int ring_size_ok(uint32_t N) {
    if (N < fhe::RING_N_MIN || N > fhe::RING_N_MAX || (N & (N - 1))) return fhe::fail("ring transform: the size must be a power of two in 4 .. 32768");
    return 0;
}

int fhe_ring_ntt_host(uint32_t N, int inverse, uint32_t* polys, uint32_t count) {
    if (count && !polys) return fhe::fail("null pointer");
    if (ring_size_ok(N)) return 1;
    try {
        fhe::RingTables tb;
        fhe::ring_tables(N, &tb);
        for (size_t x = 0; x < (size_t)count * N; x++)
            if (polys[x] >= fhe::RING_P) return fhe::fail("ring transform: a residue is not below P");
        for (uint32_t x = 0; x < count; x++) (inverse ? fhe::ring_ntt_inverse : fhe::ring_ntt_forward)(tb, polys + (size_t)x * N);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_ring_product_host(uint32_t N, uint32_t terms, const int32_t* a, const int32_t* b, int64_t* out) {
    if (!a || !b || !out) return fhe::fail("null pointer");
    if (ring_size_ok(N)) return 1;
    try {
        fhe::RingTables tb;
        fhe::ring_tables(N, &tb);
        fhe::ring_product(tb, terms, a, b, out);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

// ---- narrow packed results (glwe_narrow.h) ----
int fhe_narrow_noise(const fhe_params_t* params, const fhe_packing_params_t* pp, uint32_t bits, double out[3]) {
    if (!params || !pp || !out) return fhe::fail("null pointer");
    out[0] = out[1] = out[2] = 0;
    if (!fhe::narrow_bits_ok(bits)) return fhe::fail("narrow: the width must be 8 .. 32 bits");
    if (fhe::packing_params_check(*params, *pp)) return 1;
    fhe::narrow_noise(*params, *pp, bits, out);
    return 0;
}

int fhe_narrow_default_bits(const fhe_params_t* params, const fhe_packing_params_t* pp, int operand, uint32_t* bits) {
    if (!params || !pp || !bits) return fhe::fail("null pointer");
    *bits = 0;
    if (fhe::packing_params_check(*params, *pp)) return 1;
    double v[3], target;
    fhe::packed_log2_pfail(*params, *pp, 0.0, &target);
    for (uint32_t b = fhe::NARROW_BITS_MIN; b <= fhe::NARROW_BITS_MAX; b++) {
        fhe::narrow_noise(*params, *pp, b, v);
        if (operand ? v[0] <= v[1] : v[2] <= target) {
            *bits = b;
            return 0;
        }
    }
    return fhe::fail("narrow: no width of 8 .. 32 bits is " + std::string(operand ? "operand" : "client") + "-grade under the packing pair (" +
                     std::to_string(pp->base_log) + ", " + std::to_string(pp->level) + "): at 32 bits " +
                     (operand ? "a raw extracted block carries " + std::to_string(v[0]) + " nominal variances, the PBS-input budget is " + std::to_string(v[1])
                              : "log2 of the decoding failure probability is " + std::to_string(v[2]) + ", the bound " + std::to_string(target)));
}

size_t fhe_narrow_len(const fhe_params_t* params, uint32_t held, uint32_t bits) {
    return params ? fhe::narrow_len(params->N, params->k, held, bits) : 0;
}

static int narrow_answer(const char* why) { return why ? fhe::fail(why) : 0; }

int fhe_glwe_narrow_host(const fhe_params_t* params, const uint64_t* glwes, uint32_t held, uint32_t bits, uint64_t* narrow) {
    if (!params || (held && (!glwes || !narrow))) return fhe::fail("null pointer");
    return narrow_answer(fhe::glwe_narrow(params->N, params->k, glwes, held, bits, narrow));
}

int fhe_glwe_widen_host(const fhe_params_t* params, const uint64_t* narrow, uint32_t held, uint32_t bits, uint64_t* glwes) {
    if (!params || (held && (!glwes || !narrow))) return fhe::fail("null pointer");
    return narrow_answer(fhe::glwe_widen(params->N, params->k, narrow, held, bits, glwes));
}

int fhe_narrow_sample_extract_host(const fhe_params_t* params, const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first,
                                   uint32_t count, uint64_t* cts) {
    if (!params || (count && (!narrow || !cts))) return fhe::fail("null pointer");
    return narrow_answer(fhe::narrow_sample_extract(params->N, params->k, narrow, held, bits, first, count, cts));
}

int fhe_client_decrypt_narrow(fhe_client_key* ck, const uint64_t* narrow, uint32_t held, uint32_t bits, uint64_t* msgs) {
    if (!ck || (held && (!narrow || !msgs))) return fhe::fail("null pointer");
    try {
        const auto& c = *ck->impl;
        std::vector<uint64_t> glwes(fhe_packed_glwe_len(&c.p, held));
        if (narrow_answer(fhe::glwe_widen(c.p.N, c.p.k, narrow, held, bits, glwes.data()))) return 1;
        return fhe_client_decrypt_packed(ck, glwes.data(), held, msgs);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
}

int fhe_client_secret_keys(fhe_client_key* ck, uint64_t* glwe_sk, uint64_t* small_sk) {
    if (!ck) return fhe::fail("null pointer");
    auto& c = *ck->impl;
    if (glwe_sk) std::memcpy(glwe_sk, c.glwe_sk.data(), c.glwe_sk.size() * 8);
    if (small_sk) std::memcpy(small_sk, c.small_sk.data(), c.small_sk.size() * 8);
    return 0;
}

}  // extern "C"
