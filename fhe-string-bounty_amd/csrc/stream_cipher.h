// stream_cipher.h -- Trivium and Kreyvium in the clear: what a client encrypts its string with before the server removes the
// keystream homomorphically (transcipher.h).  Standard headers and include/fhestr.h only: no HIP, no engine, so the unit
// compiles stand-alone under a host sanitizer (tests/transcipher_main.cpp).
//
// History form.  The 288-bit state is s1 .. s288 with registers A = s1..s93, B = s94..s177, C = s178..s288; a[t], b[t], c[t]
// is the bit shifted into A, B, C at step t >= 0 and the initial contents are a[-i] = s_i, b[-i] = s_{93+i}, c[-i] = s_{177+i}.
//     z[t] = a[t-66] ^ a[t-93] ^ b[t-69] ^ b[t-84] ^ c[t-66] ^ c[t-111]          (Kreyvium: ^ K*_t)
//     a[t] = c[t-66] ^ c[t-111] ^ (c[t-109] & c[t-110]) ^ a[t-69]                (Kreyvium: ^ K*_t)
//     b[t] = a[t-66] ^ a[t-93]  ^ (a[t-91]  & a[t-92])  ^ b[t-78]                (Kreyvium: ^ IV*_t)
//     c[t] = b[t-69] ^ b[t-84]  ^ (b[t-82]  & b[t-83])  ^ c[t-87]
// with K*_t = K_{(t mod 128)+1}, IV*_t = IV_{(t mod 128)+1}.  The first 1152 steps are discarded: keystream bit i is
// z[1152 + i].  Initial state:
//     Trivium   s1..s80 = K1..K80, s94..s173 = IV1..IV80, s286..s288 = 1, the rest 0
//     Kreyvium  s1..s93 = K1..K93, s94..s177 = IV1..IV84, s178..s221 = IV85..IV128, s222..s287 = 1, s288 = 0
// Bit order (the reference's apps/trivium and the published vectors): a key or IV of L bits given as bytes is the bit
// array x[8j + l] = bit l (LSB first) of byte j, and spec bit K_j is x[L - j]; keystream bit z[8j + l] is bit l of
// keystream byte j.
//
// Trivium is an 80-bit cipher: it is here for its published vectors and for parity with the reference.  Kreyvium is the
// one whose 128-bit key matches the 128-bit parameter sets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fhestr.h"

#if defined(__HIPCC__)
#define FHE_SC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FHE_SC_HD inline
#endif

namespace fhe {

constexpr uint32_t STREAM_WARMUP_STEPS = 1152;

FHE_SC_HD bool stream_cipher_ok(uint32_t cipher) { return cipher == FHE_STREAM_TRIVIUM || cipher == FHE_STREAM_KREYVIUM; }
// key bits = IV bits: 80 (Trivium) or 128 (Kreyvium)
FHE_SC_HD uint32_t stream_key_bits(uint32_t cipher) { return cipher == FHE_STREAM_KREYVIUM ? 128 : 80; }
// spec bit j (1 .. L) of a key or IV given as L / 8 bytes
FHE_SC_HD uint32_t stream_spec_bit(const uint8_t* bytes, uint32_t L, uint32_t j) { return (bytes[(L - j) >> 3] >> ((L - j) & 7)) & 1; }

// What the register `reg` (0 = A, 1 = B, 2 = C) holds at history index -i, 1 <= i <= 128, before the first step.
constexpr uint32_t STREAM_INIT_ZERO = 0, STREAM_INIT_ONE = 1, STREAM_INIT_KEY = 2, STREAM_INIT_IV = 3;
struct StreamInit { uint32_t what, j; };   // j: the spec bit number K_j / IV_j, 1 .. L
FHE_SC_HD StreamInit stream_initial(uint32_t cipher, uint32_t reg, uint32_t i) {
    if (cipher == FHE_STREAM_KREYVIUM) {
        if (reg == 0) return i <= 93 ? StreamInit{STREAM_INIT_KEY, i} : StreamInit{STREAM_INIT_ZERO, 0};
        if (reg == 1) return i <= 84 ? StreamInit{STREAM_INIT_IV, i} : StreamInit{STREAM_INIT_ZERO, 0};
        if (i <= 44) return StreamInit{STREAM_INIT_IV, 84 + i};
        return StreamInit{i <= 110 ? STREAM_INIT_ONE : STREAM_INIT_ZERO, 0};
    }
    if (reg == 0) return i <= 80 ? StreamInit{STREAM_INIT_KEY, i} : StreamInit{STREAM_INIT_ZERO, 0};
    if (reg == 1) return i <= 80 ? StreamInit{STREAM_INIT_IV, i} : StreamInit{STREAM_INIT_ZERO, 0};
    return StreamInit{i >= 109 && i <= 111 ? STREAM_INIT_ONE : STREAM_INIT_ZERO, 0};
}

// out[0 .. n_bytes): keystream bytes first_byte .. first_byte + n_bytes - 1 under (key, iv), each L / 8 bytes.  Returns
// nullptr, or the reason it refuses; nothing is written then.
const char* stream_keystream(uint32_t cipher, const uint8_t* key, const uint8_t* iv, uint64_t first_byte, uint8_t* out, size_t n_bytes);

}  // namespace fhe
