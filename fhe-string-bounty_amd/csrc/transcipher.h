// transcipher.h -- Trivium / Kreyvium keystream generation on encrypted key bits, 64 steps per round: the definition,
// shared by the host loops (transcipher.cpp) and the kernels (transcipher_kernels.hip.h).  Includes standard headers,
// include/fhestr.h and stream_cipher.h only, so that the unit compiles stand-alone under a host sanitizer
// (tests/transcipher_main.cpp).  The cipher itself: stream_cipher.h.
//
// A state bit is a big-key LWE of the value 0 or 1 at the parameter set's delta with the noise of one PBS output; a clear
// bit (an IV bit, a constant of the initial state) is a trivial ciphertext and goes through the sums like any other row.
// Every tap of both ciphers lags by at least 66 steps, so round r computes steps 64 r .. 64 r + 63 from bits of rounds
// r - 1 and r - 2 alone: one lookup level of depth one.
//
// State update, one lookup per new bit: with s = x + y (the two ANDed taps) and t = the sum of the T XORed encrypted terms
// the PBS input is v = (T + 1) s + t and the table is
//     f_T(v) = [v div (T + 1) == 2] xor ((v mod (T + 1)) & 1)
// T = 3 everywhere except Kreyvium's a update (T = 4: it adds the encrypted K*_t; v <= 14).  The one clear XOR term,
// Kreyvium's IV*_t in the b update, is not added to the ciphertext: it selects the complemented table 1 - f_T.
// Keystream: z is the parity of the sum of its 6 taps (7 with Kreyvium's K*_t).  Bit i of a block under the clear cipher
// bit c takes the table g_{i,c}(v) = ((v & 1) xor c) << i, which removes the keystream and places the bit in one lookup; a
// string block is the sum of its `bits` = log2(msg_mod) lookups, block b of character j takes z[8 j + bits b + i]: the
// layout of string_to_blocks.
// Noise at a PBS input, in nominal variances: 2 (T + 1)^2 + T for a state update, 6 or 7 for a keystream lookup.
//
// Round block of one stream: rows 0..63 a[64 r + j], 64..127 b, 128..191 c, 192..255 the keystream lookups of steps
// 64 r + j.  Warm-up rounds (r < 18) and the two initial "rounds" -1 and -2 have the 192 state rows only.  Round blocks
// live in a ring of TC_RING = 4 slots, slot r mod 4; a slot holds S streams back to back at the row count of its round,
// which is what one ks_pbs level over S x rows inputs writes, so the lookups of round r go straight into their slot.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fhestr.h"
#include "stream_cipher.h"

#define FHE_TC_HD FHE_SC_HD

namespace fhe {

constexpr uint32_t TC_RING = 4, TC_STATE_ROWS = 192, TC_DATA_ROWS = 256, TC_WARMUP_ROUNDS = STREAM_WARMUP_STEPS / 64;
constexpr uint32_t TC_KEYSTREAM = 3;                    // row kind after the registers 0 = A, 1 = B, 2 = C
constexpr uint32_t TC_MAX_SRC = 8;                      // rows one output row sums: <= 7 in a gather, <= 8 (bits) in an apply
constexpr uint32_t TC_MAX_TABLES = 20;                  // 4 + 2 bits, bits <= 8
constexpr uint32_t TC_NONE = 0xFFFFFFFFu;
// table numbers (fhe_transcipher_table): f_3, 1 - f_3, f_4, 1 - f_4, then g_{i,c} at 4 + 2 i + c
constexpr uint32_t TC_TABLE_F3 = 0, TC_TABLE_F4 = 2, TC_TABLE_G = 4;

FHE_TC_HD uint32_t tc_reg_len(uint32_t reg) { return reg == 0 ? 93 : reg == 1 ? 84 : 111; }
FHE_TC_HD uint32_t tc_first_tap(uint32_t reg) { return reg == 1 ? 69 : 66; }     // the lag of a register's first output tap
FHE_TC_HD uint32_t tc_own_tap(uint32_t reg) { return 69 + 9 * reg; }             // the lag of the register's own feedback tap
FHE_TC_HD uint32_t tc_round_rows(int32_t round) { return round >= (int32_t)TC_WARMUP_ROUNDS ? TC_DATA_ROWS : TC_STATE_ROWS; }
FHE_TC_HD uint32_t tc_slot(int32_t round) { return (uint32_t)(round + 4) & (TC_RING - 1); }   // round >= -2
FHE_TC_HD size_t tc_slot_row(uint32_t S, int32_t round) { return (size_t)tc_slot(round) * S * TC_DATA_ROWS; }
FHE_TC_HD size_t tc_ring_rows(uint32_t S) { return (size_t)TC_RING * S * TC_DATA_ROWS; }
// ring row of kind[t] of stream s of S, t >= -128: kind 0..2 a state bit, TC_KEYSTREAM the keystream lookup of step t
FHE_TC_HD size_t tc_ring_row(uint32_t S, uint32_t s, uint32_t kind, int32_t t) {
    const uint32_t u = (uint32_t)(t + 128);
    const int32_t round = (int32_t)(u >> 6) - 2;
    return tc_slot_row(S, round) + (size_t)s * tc_round_rows(round) + kind * 64 + (u & 63);
}

// What row `kind` of step t >= 0 sums: n state rows (kind[i] at step[i]), the first n_and of them times mul, plus key row
// key_row if it is not TC_NONE.  iv_j: the spec number of the clear IV bit that complements the table, or TC_NONE.
struct TcSources {
    uint32_t n, n_and, mul, key_row, iv_j;
    uint32_t kind[6];
    int32_t step[6];
};
FHE_TC_HD TcSources tc_sources(uint32_t cipher, uint32_t kind, int32_t t) {
    const bool kreyvium = cipher == FHE_STREAM_KREYVIUM;
    TcSources r{};
    r.key_row = r.iv_j = TC_NONE;
    if (kind == TC_KEYSTREAM) {
        r.n = 6; r.n_and = 0; r.mul = 1;
        for (uint32_t reg = 0; reg < 3; reg++) {
            r.kind[2 * reg] = r.kind[2 * reg + 1] = reg;
            r.step[2 * reg] = t - (int32_t)tc_first_tap(reg);
            r.step[2 * reg + 1] = t - (int32_t)tc_reg_len(reg);
        }
        if (kreyvium) r.key_row = (uint32_t)t & 127;
        return r;
    }
    const uint32_t src = (kind + 2) % 3, len = tc_reg_len(src);         // a <- c, b <- a, c <- b
    r.n = 5; r.n_and = 2;
    r.kind[0] = r.kind[1] = r.kind[2] = r.kind[3] = src; r.kind[4] = kind;
    r.step[0] = t - (int32_t)(len - 2); r.step[1] = t - (int32_t)(len - 1);
    r.step[2] = t - (int32_t)tc_first_tap(src); r.step[3] = t - (int32_t)len;
    r.step[4] = t - (int32_t)tc_own_tap(kind);
    if (kreyvium && kind == 0) r.key_row = (uint32_t)t & 127;          // K*_t = K_{(t mod 128) + 1}: row t mod 128 of K_1 .. K_128
    if (kreyvium && kind == 1) r.iv_j = ((uint32_t)t & 127) + 1;
    r.mul = (r.key_row != TC_NONE ? 4 : 3) + 1;
    return r;
}
// the table of a state row: by T and by the clear term
FHE_TC_HD uint32_t tc_state_table(const TcSources& r, uint32_t clear_bit) { return (r.mul == 5 ? TC_TABLE_F4 : TC_TABLE_F3) + (clear_bit & 1); }
// keystream row j (0..63) of a round: bit j & 7 of its character, bit i = (j & 7) % bits of its block
FHE_TC_HD uint32_t tc_keystream_table(uint32_t j, uint32_t bits, uint32_t clear_bit) { return TC_TABLE_G + 2 * ((j & 7) % bits) + (clear_bit & 1); }
FHE_TC_HD uint64_t tc_table_value(uint32_t table, uint32_t v) {
    if (table >= TC_TABLE_G) return (uint64_t)((v & 1) ^ (table & 1)) << ((table - TC_TABLE_G) >> 1);
    const uint32_t m = table >= TC_TABLE_F4 ? 5 : 4;
    return (uint64_t)(((v / m == 2) ^ ((v % m) & 1)) ^ (table & 1));
}
// largest PBS input of a kind of row, and its noise in nominal variances
FHE_TC_HD uint32_t tc_max_input(uint32_t cipher, uint32_t kind) {
    const TcSources r = tc_sources(cipher, kind, 0);
    const uint32_t terms = r.n - r.n_and + (r.key_row != TC_NONE ? 1 : 0);
    return r.mul * r.n_and + terms;
}
FHE_TC_HD uint32_t tc_input_noise(uint32_t cipher, uint32_t kind) {
    const TcSources r = tc_sources(cipher, kind, 0);
    const uint32_t terms = r.n - r.n_and + (r.key_row != TC_NONE ? 1 : 0);
    return r.mul * r.mul * r.n_and + terms;
}

// The shape a round works on.  bits = log2(msg_mod); ivs = S x key_bits / 8 bytes; key = key_bits rows K_1 .. K_L.
struct TcShape {
    uint32_t big, bits, cipher, S;      // words of a row (kN + 1), bits per block, FHE_STREAM_*, streams
    uint64_t delta;
};
FHE_TC_HD uint32_t tc_blocks_per_char(const TcShape& sh) { return 8 / sh.bits; }
// the clear cipher bit under keystream row j of call round m (a `next` call's rounds count from 0): 0 past the call's bytes
FHE_TC_HD uint32_t tc_data_bit(const uint8_t* data, uint32_t n_bytes, uint32_t s, uint32_t m, uint32_t j) {
    const uint32_t byte = 8 * m + (j >> 3);
    return data && byte < n_bytes ? (data[(size_t)s * n_bytes + byte] >> (j & 7)) & 1 : 0;
}

// ---- host loops (transcipher.cpp): plain restatements, the pin of the kernels.  Each returns nullptr or why it refuses. ----
// nullptr if the parameter set can run the cipher, else the reason (transcipher.cpp; needs no device)
const char* tc_supported(const fhe_params_t& p, uint32_t cipher);
const char* tc_shape(const fhe_params_t& p, uint32_t cipher, uint32_t S, TcShape* out);
// ring: tc_ring_rows(S) rows; writes the blocks of rounds -1 and -2 (2 x S x 192 rows) and nothing else
const char* tc_init(const TcShape& sh, const uint64_t* key, const uint8_t* ivs, uint64_t* ring);
// pbs_in: S x rows rows, tables: S x rows table numbers mapped through lut_of (nullptr: the numbers themselves).
// rows = 192 (warm-up, data ignored) or 256; data = S x n_bytes clear cipher bytes, m the round within the call.
const char* tc_gather(const TcShape& sh, int32_t round, uint32_t rows, const uint64_t* ring, const uint64_t* key, const uint8_t* ivs,
                      const uint8_t* data, uint32_t n_bytes, uint32_t m, const uint32_t* lut_of, uint64_t* pbs_in, uint32_t* tables);
// out: S x n_bytes x blocks_per_char rows; writes the blocks of characters 8 m .. min(8 m + 8, n_bytes) - 1 of every stream
const char* tc_apply(const TcShape& sh, int32_t round, const uint64_t* ring, uint32_t n_bytes, uint32_t m, uint64_t* out);

}  // namespace fhe
