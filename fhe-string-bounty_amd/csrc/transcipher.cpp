// transcipher.cpp -- the host loops of transcipher.h: which parameter sets can run a cipher, the initial round blocks, the
// PBS inputs and table numbers of a round, and the block sums.  Plain loops over the definition; the kernels of
// transcipher_kernels.hip.h are compared with them word for word (tests/test_gpu_transcipher.py).  Stand-alone: standard
// headers, include/fhestr.h, stream_cipher.h and noise_model.h only.
#include "transcipher.h"

#include <stdio.h>
#include <string.h>

#include "noise_model.h"

namespace fhe {

namespace {

thread_local char g_reason[256];

uint32_t log2_exact(uint32_t x) {   // log2 of a power of two, else 0
    uint32_t b = 0;
    while ((1u << b) < x) b++;
    return (1u << b) == x ? b : 0;
}

void add_row(uint64_t* dst, const uint64_t* src, uint64_t mul, uint32_t big) {
    for (uint32_t w = 0; w < big; w++) dst[w] += mul * src[w];   // mod 2^64
}

}  // namespace

const char* tc_supported(const fhe_params_t& p, uint32_t cipher) {
    if (!stream_cipher_ok(cipher)) return "transcipher: unknown cipher (FHE_STREAM_TRIVIUM or FHE_STREAM_KREYVIUM)";
    const uint64_t values = (uint64_t)p.msg_mod * p.carry_mod;
    if (values < 16) {
        snprintf(g_reason, sizeof g_reason, "transcipher: a state update feeds a lookup values up to 14, the parameter set has msg_mod * carry_mod = %llu (16 needed)",
                 (unsigned long long)values);
        return g_reason;
    }
    const uint32_t bits = log2_exact(p.msg_mod);
    if (bits == 0 || 8 % bits) return "transcipher: msg_mod must be 2, 4, 16 or 256 (the bits of a block must divide a character's 8)";
    if (p.k == 0 || p.N == 0 || ((uint64_t)p.k * p.N & 1)) return "transcipher: k N must be even and positive";
    const NoiseModel m = noise_model(p);
    const double budget = default_noise_budget(p);
    for (uint32_t kind = 0; kind <= TC_KEYSTREAM; kind++) {
        const uint32_t v = tc_max_input(cipher, kind), nu = tc_input_noise(cipher, kind);
        if (v >= values) {
            snprintf(g_reason, sizeof g_reason, "transcipher: a lookup input reaches %u, the parameter set holds %llu values", v, (unsigned long long)values);
            return g_reason;
        }
        if (!((double)nu <= budget)) {
            snprintf(g_reason, sizeof g_reason, "transcipher: a lookup input carries %u nominal variances (log2 p_fail %.1f), the PBS-input budget is %.2f (log2 p_fail %.1f)",
                     nu, m.log2_pfail(nu), budget, m.log2_pfail(budget));
            return g_reason;
        }
    }
    return nullptr;
}

const char* tc_shape(const fhe_params_t& p, uint32_t cipher, uint32_t S, TcShape* out) {
    if (const char* why = tc_supported(p, cipher)) return why;
    if (S == 0 || S > 4096) return "transcipher: 1 .. 4096 streams";
    out->big = p.k * p.N + 1;
    out->bits = log2_exact(p.msg_mod);
    out->cipher = cipher;
    out->S = S;
    out->delta = (1ull << 63) / ((uint64_t)p.msg_mod * p.carry_mod);
    return nullptr;
}

const char* tc_init(const TcShape& sh, const uint64_t* key, const uint8_t* ivs, uint64_t* ring) {
    const uint32_t L = stream_key_bits(sh.cipher);
    for (uint32_t s = 0; s < sh.S; s++)
        for (uint32_t reg = 0; reg < 3; reg++)
            for (uint32_t i = 1; i <= 128; i++) {
                uint64_t* row = ring + tc_ring_row(sh.S, s, reg, -(int32_t)i) * sh.big;
                const StreamInit si = stream_initial(sh.cipher, reg, i);
                if (si.what == STREAM_INIT_KEY) { memcpy(row, key + (size_t)(si.j - 1) * sh.big, (size_t)sh.big * 8); continue; }
                memset(row, 0, (size_t)sh.big * 8);
                const uint32_t bit = si.what == STREAM_INIT_IV ? stream_spec_bit(ivs + (size_t)s * (L / 8), L, si.j) : si.what;
                row[sh.big - 1] = bit * sh.delta;
            }
    return nullptr;
}

const char* tc_gather(const TcShape& sh, int32_t round, uint32_t rows, const uint64_t* ring, const uint64_t* key, const uint8_t* ivs,
                      const uint8_t* data, uint32_t n_bytes, uint32_t m, const uint32_t* lut_of, uint64_t* pbs_in, uint32_t* tables) {
    if (round < 0 || round > (1 << 24)) return "transcipher: round out of range";
    if (rows != TC_STATE_ROWS && rows != TC_DATA_ROWS) return "transcipher: a round has 192 or 256 rows";
    const uint32_t L = stream_key_bits(sh.cipher);
    for (uint32_t s = 0; s < sh.S; s++)
        for (uint32_t row = 0; row < rows; row++) {
            const uint32_t kind = row >> 6, j = row & 63;
            const TcSources src = tc_sources(sh.cipher, kind, 64 * round + (int32_t)j);
            uint64_t* dst = pbs_in + ((size_t)s * rows + row) * sh.big;
            memset(dst, 0, (size_t)sh.big * 8);
            for (uint32_t i = 0; i < src.n; i++)
                add_row(dst, ring + tc_ring_row(sh.S, s, src.kind[i], src.step[i]) * sh.big, i < src.n_and ? src.mul : 1, sh.big);
            if (src.key_row != TC_NONE) add_row(dst, key + (size_t)src.key_row * sh.big, 1, sh.big);
            uint32_t table;
            if (kind == TC_KEYSTREAM) table = tc_keystream_table(j, sh.bits, tc_data_bit(data, n_bytes, s, m, j));
            else table = tc_state_table(src, src.iv_j != TC_NONE ? stream_spec_bit(ivs + (size_t)s * (L / 8), L, src.iv_j) : 0);
            tables[(size_t)s * rows + row] = lut_of ? lut_of[table] : table;
        }
    return nullptr;
}

const char* tc_apply(const TcShape& sh, int32_t round, const uint64_t* ring, uint32_t n_bytes, uint32_t m, uint64_t* out) {
    if (round < (int32_t)TC_WARMUP_ROUNDS) return "transcipher: a warm-up round has no keystream rows";
    const uint32_t bpc = tc_blocks_per_char(sh);
    for (uint32_t s = 0; s < sh.S; s++)
        for (uint32_t ch = 8 * m; ch < 8 * m + 8 && ch < n_bytes; ch++)
            for (uint32_t b = 0; b < bpc; b++) {
                uint64_t* dst = out + (((size_t)s * n_bytes + ch) * bpc + b) * sh.big;
                memset(dst, 0, (size_t)sh.big * 8);
                for (uint32_t i = 0; i < sh.bits; i++)
                    add_row(dst, ring + tc_ring_row(sh.S, s, TC_KEYSTREAM, 64 * round + (int32_t)(8 * (ch - 8 * m) + sh.bits * b + i)) * sh.big, 1, sh.big);
            }
    return nullptr;
}

}  // namespace fhe
