// glwe_narrow.h -- packed GLWE results at b-bit coefficients: the definition, shared by the host loops (glwe_narrow.cpp)
// and the kernels (glwe_narrow_kernels.hip.h).  Includes standard headers and include/fhestr.h only, so that the unit
// compiles stand-alone under a host sanitizer (tests/narrow_main.cpp).
//
// The project's own form (include/fhestr.h, "narrow packed results"; the reference has no counterpart).  For a width
// 8 <= b <= 32:
//     narrow_b(x) = ((x + 2^(63-b)) >> (64-b)) mod 2^b      round to nearest, ties upwards; the top wraps to 0
//     widen_b(v)  = v << (64-b)
// A packed list of `held` blocks has G = ceil(held / N) GLWEs of [k+1][N] u64; GLWE g holds m_g = min(N, held - g N) blocks.
// Its narrow form is a bit stream of kN + m_g fields of b bits: field f is narrow_b of word f of the GLWE (the body follows
// the mask, so the fields are its first kN + m_g words), bit t of the stream is bit t & 63 of u64 word t >> 6, the unused
// high bits of the last word are 0.  Stream g starts at word g W of the list, W = ceil((kN + N) b / 64); the last stream
// has ceil((kN + m_g) b / 64) words only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fhestr.h"

#if defined(__HIPCC__)
#define FHE_NARROW_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FHE_NARROW_HD inline
#endif

namespace fhe {

constexpr uint32_t NARROW_BITS_MIN = 8, NARROW_BITS_MAX = 32;

FHE_NARROW_HD bool narrow_bits_ok(uint32_t b) { return b >= NARROW_BITS_MIN && b <= NARROW_BITS_MAX; }
FHE_NARROW_HD uint64_t narrow_word(uint64_t x, uint32_t b) { return (x + (1ull << (63 - b))) >> (64 - b); }   // the sum wraps mod 2^64
// v < 2^b <= 2^32: the low half of the result is 0, so the shift is a 32-bit one
FHE_NARROW_HD uint64_t widen_word(uint32_t v, uint32_t b) { return (uint64_t)(v << (32 - b)) << 32; }

// u64 words of a stream of `fields` fields
FHE_NARROW_HD size_t narrow_stream_words(size_t fields, uint32_t b) { return (fields * b + 63) / 64; }
// blocks GLWE g of a list of `held` holds; g < ceil(held / N)
FHE_NARROW_HD uint32_t narrow_blocks_of(uint32_t N, uint32_t held, uint32_t g) {
    const uint64_t left = (uint64_t)held - (uint64_t)g * N;
    return left < N ? (uint32_t)left : N;
}

// Field f of a stream given as `len32` 32-bit words (little endian: u32 word w is half w & 1 of u64 word w >> 1).  Reads
// the word the field starts in, and the next one only when the field crosses into it -- a field of <= 32 bits touches at
// most two -- and never a word at or past len32: for every field of a well-formed stream both lie inside it.
// 32-bit index arithmetic, the hot path of narrow_sample_extract_kernel: a stream has (k + 1) N < 2^27 fields
// (narrow_len refuses larger shapes), so its bit offsets stay below 2^32.
FHE_NARROW_HD uint32_t narrow_field(const uint32_t* s, uint32_t len32, uint32_t f, uint32_t b) {
    const uint32_t bit = f * b, w = bit >> 5, sh = bit & 31;
    uint32_t v = w < len32 ? s[w] >> sh : 0;
    if (sh + b > 32 && w + 1 < len32) v |= s[w + 1] << (32 - sh);   // sh >= 1 here
    return b == 32 ? v : v & ((1u << b) - 1);
}

// Index of the field behind word j (j <= k N) of the LWE at coefficient c: polynomial j / N, coefficient c - i mod N with
// i = j % N (glwe_row_word of glwe_extract_kernels.hip.h); the word is negated when i > c.  N a power of two.
FHE_NARROW_HD uint32_t narrow_row_field(uint32_t N, uint32_t c, uint32_t j) {
    const uint32_t i = j & (N - 1);
    return (j - i) + ((c - i) & (N - 1));
}

// ---- host loops (glwe_narrow.cpp).  Each returns nullptr, or the reason it refuses; nothing is touched then. ----
// u64 words of the narrow list; 0 when refused (bits out of range, N not a power of two >= 2, k < 1, (k + 1) N >= 2^27)
size_t narrow_len(uint32_t N, uint32_t k, uint32_t held, uint32_t bits);
// glwes: ceil(held / N) x [k+1][N] -> out: narrow_len words, every one written
const char* glwe_narrow(uint32_t N, uint32_t k, const uint64_t* glwes, uint32_t held, uint32_t bits, uint64_t* out);
// narrow: narrow_len words -> glwes: ceil(held / N) x [k+1][N], the body coefficients that hold no block 0
const char* glwe_widen(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits, uint64_t* glwes);
// blocks first .. first + count - 1 -> cts: count x (kN + 1); equals sample extraction of glwe_widen's output word for word
const char* narrow_sample_extract(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first,
                                  uint32_t count, uint64_t* cts);
// nullptr if every unused high bit of every stream's last word is 0, else the reason
const char* narrow_tail_check(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits);

}  // namespace fhe
