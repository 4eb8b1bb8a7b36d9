// glwe_narrow_kernels.hip.h -- packed GLWE results at b-bit coefficients on the device (the definition: glwe_narrow.h).
//
// glwe_narrow_kernel: full GLWEs [.][k+1][N] -> the narrow list.  One thread builds one output u64 from the <= 64 / b + 2
// source words whose fields overlap it (9 at b = 8, 3 at b = 32): consecutive lanes read consecutive runs of the GLWE and
// store consecutive words.  A field that straddles two output words is rounded by both threads -- the same integer
// expression -- so no atomics and no LDS; fields past a stream's last are never read, which leaves its tail bits 0.
//
// narrow_sample_extract_kernel: glwe_sample_extract_kernel (glwe_extract_kernels.hip.h) reading straight from the narrow
// list.  The store shape is that kernel's, unchanged: rows of kN + 1 words as aligned 16-byte pairs plus the one word the
// pairs leave out, the row's parity taken from the destination address, GLWE_EXTRACT_PAIRS_PER_WG pairs per workgroup.
// Per word: the field index as glwe_row_word computes it, the field through the reader the host loop uses
// (narrow_field: one 32-bit load, a second only when the field crosses into the next word), shifted left by 64 - b and
// negated by a select when i > c -- exact mod 2^64, so the rows equal sample extraction of the widened GLWEs word for
// word.  All of it is 32-bit arithmetic: a stream's bit offsets stay below 2^32 and a widened word's low half is 0.
// Still write-bound: 8 (kN + 1) bytes out per row; the narrow stream of one GLWE is (k + 1) N b / 8 bytes (8 KB at
// N = 2048, b = 16) and its N rows re-read it from L2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glwe_extract_kernels.hip.h"
#include "glwe_narrow.h"

namespace fhe {

constexpr uint32_t FHE_NARROW_KERNEL_NARROW = 1, FHE_NARROW_KERNEL_EXTRACT = 2, FHE_NARROW_KERNEL_WIDEN = 3;   // fhe_engine_narrow_info's info[1]

// glwes = [n_glwe][k+1][N], out = the narrow list of `held` blocks, `words` = narrow_len u64 words in all, stride = u64
// words between two streams.  grid = ceil(words / 256).
__global__ void __launch_bounds__(256) glwe_narrow_kernel(const uint64_t* __restrict__ glwes, uint64_t* __restrict__ out, uint32_t N, uint32_t kN,
                                                          uint32_t held, uint32_t bits, uint32_t stride, uint64_t words) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const uint32_t g = (uint32_t)(idx / stride), t = (uint32_t)(idx % stride);
    const uint32_t fields = kN + narrow_blocks_of(N, held, g);              // <= kN + N: inside GLWE g
    const uint64_t* __restrict__ src = glwes + (size_t)g * ((size_t)kN + N);
    const uint64_t lo = (uint64_t)t * 64, hi = lo + 63;                     // the stream bits this word holds
    uint32_t f = (uint32_t)(lo / bits);
    const uint32_t f_last = (uint32_t)(hi / bits);
    uint64_t w = 0;
    for (; f <= f_last && f < fields; f++) {
        const uint64_t v = narrow_word(src[f], bits);
        const int64_t pos = (int64_t)((uint64_t)f * bits) - (int64_t)lo;   // -bits < pos < 64
        w |= pos < 0 ? v >> (uint32_t)(-pos) : v << (uint32_t)pos;
    }
    out[idx] = w;
}

// The narrow list of `held` blocks -> full GLWEs [n_glwe][k+1][N], the body coefficients that hold no block 0: one thread
// per GLWE word, consecutive lanes store consecutive words.  The first step of the two-step route (widen in HBM, then
// glwe_sample_extract_kernel) that scripts/glwe_narrow_timing.py times next to the fused extraction; also what a caller
// uses who wants the full GLWEs on the device.  grid = ceil(n_glwe (k+1) N / 256).
__global__ void __launch_bounds__(256) glwe_widen_kernel(const uint64_t* __restrict__ narrow, uint64_t* __restrict__ glwes, uint32_t N, uint32_t kN,
                                                         uint32_t held, uint32_t bits, uint32_t stride, uint64_t words) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;                               // words = n_glwe (kN + N)
    const uint32_t glwe_len = kN + N, g = (uint32_t)(idx / glwe_len), f = (uint32_t)(idx % glwe_len);
    const uint32_t fields = kN + narrow_blocks_of(N, held, g);
    const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(narrow + (size_t)g * stride);
    glwes[idx] = f < fields ? widen_word(narrow_field(s, 2 * (uint32_t)narrow_stream_words(fields, bits), f, bits), bits) : 0;
}

// word j of the row (j <= k N) at coefficient c, from one GLWE's stream of len32 32-bit words
__device__ __forceinline__ uint64_t narrow_row_word(const uint32_t* __restrict__ s, uint32_t len32, uint32_t N, uint32_t c, uint32_t j, uint32_t bits) {
    const uint32_t hi = narrow_field(s, len32, narrow_row_field(N, c, j), bits) << (32 - bits);   // widen_word's high half; the low half is 0
    return (uint64_t)((j & (N - 1)) > c ? 0u - hi : hi) << 32;                                      // so the negation mod 2^64 is one of the high half
}

// narrow = the list of `held` blocks (first + count <= held, checked by the host), out = [count][kN + 1]; N a power of
// two, kN even.  grid = count * chunks workgroups, chunks = ceil(kN / 2 / GLWE_EXTRACT_PAIRS_PER_WG).
__global__ void __launch_bounds__(256) narrow_sample_extract_kernel(const uint64_t* __restrict__ narrow, uint64_t* __restrict__ out, uint32_t N,
                                                                    uint32_t kN, uint32_t held, uint32_t bits, uint32_t stride, uint32_t first,
                                                                    uint32_t count, uint32_t chunks) {
    const uint32_t row = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (row >= count) return;
    const uint32_t block = first + row;                     // < held
    const uint32_t c = block & (N - 1), g = block / N;
    const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(narrow + (size_t)g * stride);
    const uint32_t len32 = 2 * (uint32_t)narrow_stream_words((size_t)kN + narrow_blocks_of(N, held, g), bits);
    uint64_t* __restrict__ dst = out + (size_t)row * ((size_t)kN + 1);
    const uint32_t o = (uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 3) & 1;   // words to the next 16-byte boundary
    const uint32_t pairs = kN / 2;
    const uint32_t p_lo = chunk * GLWE_EXTRACT_PAIRS_PER_WG;
    const uint32_t p_hi = p_lo + GLWE_EXTRACT_PAIRS_PER_WG < pairs ? p_lo + GLWE_EXTRACT_PAIRS_PER_WG : pairs;
#pragma unroll 4
    for (uint32_t q = p_lo + threadIdx.x; q < p_hi; q += 256) {
        const uint32_t j = o + 2 * q;                          // j + 1 <= kN
        GlweExtractPair w;
        w.lo = narrow_row_word(s, len32, N, c, j, bits);
        w.hi = narrow_row_word(s, len32, N, c, j + 1, bits);
        *reinterpret_cast<GlweExtractPair*>(dst + j) = w;      // 16-byte aligned by the choice of o
    }
    if (chunk == 0 && threadIdx.x == 0) {
        const uint32_t j = o ? 0 : kN;
        dst[j] = narrow_row_word(s, len32, N, c, j, bits);
    }
}

}  // namespace fhe
