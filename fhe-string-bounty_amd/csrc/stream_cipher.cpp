// stream_cipher.cpp -- the clear keystream of stream_cipher.h: one plain loop over the history form, one step at a time.
// Each register's history lives in a ring of 128 bits: the longest lag is 111, so the bit a step overwrites is never read
// again.  Stand-alone: standard headers and include/fhestr.h only.
#include "stream_cipher.h"

namespace fhe {

namespace {

struct History {
    uint8_t bit[128];
    uint8_t& operator[](int64_t t) { return bit[(uint64_t)(t + 128) & 127]; }   // t >= -128
};

}  // namespace

const char* stream_keystream(uint32_t cipher, const uint8_t* key, const uint8_t* iv, uint64_t first_byte, uint8_t* out, size_t n_bytes) {
    if (!stream_cipher_ok(cipher)) return "stream cipher: unknown cipher (FHE_STREAM_TRIVIUM or FHE_STREAM_KREYVIUM)";
    if (first_byte > (1ull << 56) || n_bytes > (1ull << 56)) return "stream cipher: keystream position out of range";
    if (n_bytes == 0) return nullptr;
    const uint32_t L = stream_key_bits(cipher);
    const bool kreyvium = cipher == FHE_STREAM_KREYVIUM;
    History h[3];
    for (uint32_t reg = 0; reg < 3; reg++)
        for (uint32_t i = 1; i <= 128; i++) {
            const StreamInit s = stream_initial(cipher, reg, i);
            h[reg][-(int64_t)i] = s.what == STREAM_INIT_KEY ? stream_spec_bit(key, L, s.j) : s.what == STREAM_INIT_IV ? stream_spec_bit(iv, L, s.j) : s.what;
        }
    History &a = h[0], &b = h[1], &c = h[2];
    const int64_t lo = STREAM_WARMUP_STEPS + 8 * (int64_t)first_byte, hi = lo + 8 * (int64_t)n_bytes;
    for (size_t i = 0; i < n_bytes; i++) out[i] = 0;
    for (int64_t t = 0; t < hi; t++) {
        const uint32_t ta = a[t - 66] ^ a[t - 93], tb = b[t - 69] ^ b[t - 84], tc = c[t - 66] ^ c[t - 111];
        const uint32_t ks = kreyvium ? stream_spec_bit(key, L, (uint32_t)(t & 127) + 1) : 0;
        const uint32_t ivs = kreyvium ? stream_spec_bit(iv, L, (uint32_t)(t & 127) + 1) : 0;
        const uint32_t z = ta ^ tb ^ tc ^ ks;
        const uint32_t na = tc ^ (c[t - 109] & c[t - 110]) ^ a[t - 69] ^ ks;
        const uint32_t nb = ta ^ (a[t - 91] & a[t - 92]) ^ b[t - 78] ^ ivs;
        const uint32_t nc = tb ^ (b[t - 82] & b[t - 83]) ^ c[t - 87];
        a[t] = (uint8_t)na; b[t] = (uint8_t)nb; c[t] = (uint8_t)nc;
        if (t >= lo) out[(t - lo) >> 3] |= (uint8_t)(z << ((t - lo) & 7));
    }
    return nullptr;
}

}  // namespace fhe
