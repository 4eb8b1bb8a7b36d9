// glwe_narrow.cpp -- the host loops of glwe_narrow.h: narrow, widen, sample extraction straight from the narrow list, its
// length and the tail-bit check.  Plain loops over the definition; the kernels of glwe_narrow_kernels.hip.h are pinned
// against the same exact integers (tests/exact_narrow.py).  Stand-alone: standard headers and include/fhestr.h only.
#include "glwe_narrow.h"

#include <string.h>

namespace fhe {

namespace {

const char* shape_refused(uint32_t N, uint32_t k, uint32_t bits) {
    if (!narrow_bits_ok(bits)) return "narrow: the width must be 8 .. 32 bits";
    if (N < 2 || (N & (N - 1))) return "narrow: polynomial size must be a power of two >= 2";
    if (k < 1) return "narrow: k >= 1";
    if (((uint64_t)k + 1) * N >= (1ull << 27)) return "narrow: (k + 1) N must be below 2^27";   // narrow_field's 32-bit offsets
    return nullptr;
}

struct Geometry {
    size_t kN, glwe_len, stride;   // mask words, words of a full GLWE, u64 words between two streams
    uint32_t n_glwe;
    Geometry(uint32_t N, uint32_t k, uint32_t held, uint32_t bits)
        : kN((size_t)k * N), glwe_len(kN + N), stride(narrow_stream_words(kN + N, bits)), n_glwe((uint32_t)(((uint64_t)held + N - 1) / N)) {}
};

}  // namespace

size_t narrow_len(uint32_t N, uint32_t k, uint32_t held, uint32_t bits) {
    if (shape_refused(N, k, bits) || held == 0) return 0;
    const Geometry g(N, k, held, bits);
    return (size_t)(g.n_glwe - 1) * g.stride + narrow_stream_words(g.kN + narrow_blocks_of(N, held, g.n_glwe - 1), bits);
}

const char* glwe_narrow(uint32_t N, uint32_t k, const uint64_t* glwes, uint32_t held, uint32_t bits, uint64_t* out) {
    if (const char* why = shape_refused(N, k, bits)) return why;
    const Geometry geo(N, k, held, bits);
    for (uint32_t g = 0; g < geo.n_glwe; g++) {
        const size_t fields = geo.kN + narrow_blocks_of(N, held, g);
        const uint64_t* src = glwes + (size_t)g * geo.glwe_len;
        uint64_t* dst = out + (size_t)g * geo.stride;
        memset(dst, 0, narrow_stream_words(fields, bits) * 8);
        for (size_t f = 0; f < fields; f++) {
            const uint64_t v = narrow_word(src[f], bits);
            const size_t bit = f * bits, w = bit >> 6;
            const uint32_t sh = (uint32_t)(bit & 63);
            dst[w] |= v << sh;
            if (sh + bits > 64) dst[w + 1] |= v >> (64 - sh);   // sh >= 33 here; the field's last bit lies inside the stream
        }
    }
    return nullptr;
}

const char* glwe_widen(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits, uint64_t* glwes) {
    if (const char* why = shape_refused(N, k, bits)) return why;
    const Geometry geo(N, k, held, bits);
    for (uint32_t g = 0; g < geo.n_glwe; g++) {
        const uint32_t fields = (uint32_t)geo.kN + narrow_blocks_of(N, held, g), len32 = 2 * (uint32_t)narrow_stream_words(fields, bits);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(narrow + (size_t)g * geo.stride);
        uint64_t* dst = glwes + (size_t)g * geo.glwe_len;
        for (uint32_t f = 0; f < fields; f++) dst[f] = widen_word(narrow_field(s, len32, f, bits), bits);
        for (size_t f = fields; f < geo.glwe_len; f++) dst[f] = 0;
    }
    return nullptr;
}

const char* narrow_sample_extract(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first,
                                  uint32_t count, uint64_t* cts) {
    if (const char* why = shape_refused(N, k, bits)) return why;
    if ((uint64_t)first + count > held) return "narrow: first + count exceeds the blocks the list holds";
    const Geometry geo(N, k, held, bits);
    for (uint32_t r = 0; r < count; r++) {
        const uint32_t block = first + r, g = block / N, c = block & (N - 1);
        const uint32_t len32 = 2 * (uint32_t)narrow_stream_words(geo.kN + narrow_blocks_of(N, held, g), bits);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(narrow + (size_t)g * geo.stride);
        uint64_t* ct = cts + (size_t)r * (geo.kN + 1);
        for (uint32_t j = 0; j <= geo.kN; j++) {
            const uint64_t v = widen_word(narrow_field(s, len32, narrow_row_field(N, c, j), bits), bits);
            ct[j] = (j & (N - 1)) > c ? 0 - v : v;
        }
    }
    return nullptr;
}

const char* narrow_tail_check(uint32_t N, uint32_t k, const uint64_t* narrow, uint32_t held, uint32_t bits) {
    if (const char* why = shape_refused(N, k, bits)) return why;
    const Geometry geo(N, k, held, bits);
    for (uint32_t g = 0; g < geo.n_glwe; g++) {
        const size_t used = (geo.kN + narrow_blocks_of(N, held, g)) * bits;
        if ((used & 63) && (narrow[(size_t)g * geo.stride + (used >> 6)] >> (used & 63))) return "narrow: a bit past a stream's last field is set";
    }
    return nullptr;
}

}  // namespace fhe
