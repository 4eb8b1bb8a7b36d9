// compact_pk.cpp -- the public-key side of the client: compact LWE public keys and compact ciphertext lists
// (M. Joye, eprint 2023/603, as tfhe-rs 0.5 implements it: shortint/public_key/compact.rs,
// core_crypto/algorithms/lwe_compact_public_key_generation.rs:15-50, lwe_encryption.rs:1837-1958,
// lwe_compact_ciphertext_list_expansion.rs:12-58, entities/lwe_compact_ciphertext_list.rs:41-63).  CPU code, like the
// rest of the client; the server's half -- the expansion -- runs on the device (compact_kernels.hip.h) and has its
// host twin here.
//
// n = k*N is the dimension of the big key, which must be a power of two (compact.rs:65).  All arithmetic wraps mod 2^64.
//   conv(lhs, rhs) = lhs * reverse(rhs) in Z[X]/(X^n + 1)        slice_semi_reverse_negacyclic_convolution,
//                                                                 slice_algorithms.rs:610-659
//   public key     a uniform, b = conv(a, s) + e                  2n words: a then b
//   list, per bin of at most n plaintexts: r uniform binary;  A = conv(a, r) + e1;
//                  body c = conv(b, r)[c] + e2[c] + delta * (m mod msg_mod)
//   container      all bin masks, then all bodies
//   expansion      ciphertext i = (A_{i / n} * X^{n - (i mod n + 1)}, body i)
// The right-hand side of every convolution is binary, so a convolution is one shifted, sign-folded vector add per set
// bit: exact, n^2 / 2 wrapping adds, split over threads by output range.  No FFT: the results must be exact.
// Noise: e, e1 and e2 all have the big key's standard deviation (glwe_std), as compact.rs:102-116 passes it for a
// single ciphertext; its list path hands lwe_modular_std_dev to the bodies (compact.rs:169-177), which under big-key
// encryption would put keyswitch-sized noise (2^47 under PARAM_MESSAGE_2_CARRY_2) on a fresh ciphertext.
// Randomness: ChaCha20 under the caller's 256-bit seed (det_math.h), one stream per purpose and bin, so a seed
// reproduces keys and lists bit for bit whatever the thread count.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "det_math.h"
#include "engine.h"

namespace fhe {

namespace {

constexpr uint64_t STREAM_PK_MASK = 0x43504B0000000000ull;    // "CPK": public-key mask, + 1: its noise
constexpr uint64_t STREAM_R = 0x4350520000000000ull;          // "CPR" + bin
constexpr uint64_t STREAM_E1 = 0x4350310000000000ull;         // "CP1" + bin
constexpr uint64_t STREAM_E2 = 0x4350320000000000ull;         // "CP2" + bin

bool power_of_two(uint64_t n) { return n >= 2 && (n & (n - 1)) == 0; }

// positions of the non-zero entries of the right-hand side (a 0/1 vector everywhere but in fhe_compact_conv)
std::vector<uint32_t> set_positions(const uint64_t* rhs, size_t n) {
    std::vector<uint32_t> set;
    for (size_t t = 0; t < n; t++)
        if (rhs[t]) set.push_back((uint32_t)t);
    return set;
}

// out[j] = conv(lhs, rhs)[j] for j in [lo, hi): entry t of the right-hand side contributes rhs[t] * lhs * X^(n - 1 - t)
void conv_range(uint64_t* out, const uint64_t* lhs, const uint64_t* rhs, const std::vector<uint32_t>& set, size_t n, size_t lo, size_t hi) {
    std::memset(out + lo, 0, (hi - lo) * 8);
    for (const uint32_t t : set) {
        const size_t m = n - 1 - t, split = std::min(std::max(m, lo), hi);
        const uint64_t w = rhs[t];
        if (w == 1) {
            for (size_t j = lo; j < split; j++) out[j] -= lhs[j + n - m];
            for (size_t j = split; j < hi; j++) out[j] += lhs[j - m];
        } else {
            for (size_t j = lo; j < split; j++) out[j] -= w * lhs[j + n - m];
            for (size_t j = split; j < hi; j++) out[j] += w * lhs[j - m];
        }
    }
}

struct ConvJob {
    uint64_t* out;
    const uint64_t* lhs;
    size_t hi;          // entries [0, hi) of the result are wanted
};

// several convolutions against the same right-hand side, cut into cache-sized output tiles dealt round-robin to threads
void conv_many(const std::vector<ConvJob>& jobs, const uint64_t* rhs, size_t n, int threads) {
    const std::vector<uint32_t> set = set_positions(rhs, n);
    threads = std::max(1, std::min(threads, 64));
    const size_t tile = std::max<size_t>(64, std::min<size_t>(1024, n / (size_t)threads));
    struct Tile { const ConvJob* job; size_t lo, hi; };
    std::vector<Tile> tiles;
    for (const auto& job : jobs)
        for (size_t lo = 0; lo < job.hi; lo += tile) tiles.push_back({&job, lo, std::min(job.hi, lo + tile)});
    auto run = [&](int t) {
        for (size_t i = (size_t)t; i < tiles.size(); i += (size_t)threads) conv_range(tiles[i].job->out, tiles[i].job->lhs, rhs, set, n, tiles[i].lo, tiles[i].hi);
    };
    if (threads == 1 || tiles.size() < 2) {
        for (int t = 0; t < threads; t++) run(t);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(run, t);
    for (auto& th : pool) th.join();
}

}  // namespace

size_t compact_dim(const fhe_params_t& p) {
    const uint64_t n = (uint64_t)p.k * p.N;
    return power_of_two(n) && n <= (1ull << 31) ? (size_t)n : 0;
}

int compact_pk_generate(const fhe_params_t& p, const uint64_t* big_sk, const Seed256& seed, uint64_t* pk, int threads) {
    const size_t n = compact_dim(p);
    if (!n) return fail("a compact public key needs a power-of-two encryption key dimension, k*N = " + std::to_string((uint64_t)p.k * p.N));
    uint64_t *a = pk, *b = pk + n;
    Rng mask(seed, STREAM_PK_MASK), noise(seed, STREAM_PK_MASK + 1);
    for (size_t i = 0; i < n; i++) a[i] = mask.next();
    conv_many({{b, a, n}}, big_sk, n, threads);
    for (size_t i = 0; i < n; i++) b[i] += gaussian_torus(noise, p.glwe_std);
    return 0;
}

}  // namespace fhe

extern "C" {

size_t fhe_compact_pk_len(const fhe_params_t* p) { return p ? 2 * fhe::compact_dim(*p) : 0; }

size_t fhe_compact_list_len(const fhe_params_t* p, uint32_t count) {
    const size_t n = p ? fhe::compact_dim(*p) : 0;
    return n ? ((size_t)count + n - 1) / n * n + count : 0;
}

int fhe_compact_pk_encrypt(const fhe_params_t* p, const uint64_t* pk, const uint8_t seed[32], const uint64_t* msgs, uint32_t count,
                           uint64_t* list_out, int threads) {
    if (!p || !pk || !seed || (count && (!msgs || !list_out))) return fhe::fail("null pointer");
    const size_t n = fhe::compact_dim(*p);
    if (!n) return fhe::fail("compact encryption needs a power-of-two encryption key dimension, k*N = " + std::to_string((uint64_t)p->k * p->N));
    if (p->msg_mod == 0 || p->carry_mod == 0) return fhe::fail("message and carry modulus must be positive");
    try {
        const fhe::Seed256 sd = fhe::seed_from_bytes(seed);
        const uint64_t delta = (1ull << 63) / ((uint64_t)p->msg_mod * p->carry_mod);
        const uint64_t *a = pk, *b = pk + n;
        const size_t bins = ((size_t)count + n - 1) / n;
        uint64_t* bodies = list_out + bins * n;
        std::vector<uint64_t> r(n), br(n);
        for (size_t bin = 0; bin < bins; bin++) {
            const size_t first = bin * n, in_bin = std::min(n, (size_t)count - first);
            fhe::Rng rr(sd, fhe::STREAM_R + bin), e1(sd, fhe::STREAM_E1 + bin), e2(sd, fhe::STREAM_E2 + bin);
            for (size_t i = 0; i < n; i += 64) {
                const uint64_t w = rr.next();
                for (size_t bit = 0; bit < 64 && i + bit < n; bit++) r[i + bit] = (w >> bit) & 1;
            }
            uint64_t* A = list_out + bin * n;
            fhe::conv_many({{A, a, n}, {br.data(), b, in_bin}}, r.data(), n, threads);
            for (size_t j = 0; j < n; j++) A[j] += fhe::gaussian_torus(e1, p->glwe_std);
            for (size_t c = 0; c < in_bin; c++)
                bodies[first + c] = br[c] + fhe::gaussian_torus(e2, p->glwe_std) + delta * (msgs[first + c] % p->msg_mod);
        }
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

int fhe_compact_expand_host(uint32_t lwe_dim, const uint64_t* list, uint32_t count, uint64_t* out) {
    if (count && (!list || !out)) return fhe::fail("null pointer");
    const size_t n = lwe_dim;
    if (!fhe::power_of_two(n)) return fhe::fail("compact lists need a power-of-two LWE dimension, got " + std::to_string(lwe_dim));
    const size_t bins = ((size_t)count + n - 1) / n;
    const uint64_t* bodies = list + bins * n;
    for (size_t i = 0; i < count; i++) {
        const uint64_t* A = list + i / n * n;
        uint64_t* row = out + i * (n + 1);
        const size_t d = n - (i % n + 1);
        for (size_t j = 0; j < d; j++) row[j] = 0 - A[n + j - d];
        for (size_t j = d; j < n; j++) row[j] = A[j - d];
        row[n] = bodies[i];
    }
    return 0;
}

// conv(lhs, rhs) for any rhs and any n >= 1, through the code the key generation and the encryption run (the known
// answer of slice_algorithms.rs:613-620 has n = 3 and a right-hand side that is not binary)
int fhe_compact_conv(const uint64_t* lhs, const uint64_t* rhs, uint32_t n, uint64_t* out, int threads) {
    if (!lhs || !rhs || !out) return fhe::fail("null pointer");
    if (n == 0) return fhe::fail("empty operands");
    try {
        fhe::conv_many({{out, lhs, n}}, rhs, n, threads);
    } catch (const std::exception& e) {
        return fhe::fail(e.what());
    }
    return 0;
}

}  // extern "C"
