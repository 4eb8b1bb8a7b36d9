// glwe_extract_kernels.hip.h -- packed results taken back as operation inputs: sample extraction at any coefficient.
//
// The inverse of the packing keyswitch (packing_ks_kernels.hip.h): extract_lwe_sample_from_glwe_ciphertext of the reference
// (core_crypto/algorithms/glwe_sample_extraction.rs:91-147) at coefficient c of a GLWE [k+1][N] that arrived from outside.
// The GLWE key flattened is the big LWE key, so no key is involved: row r of the output is block first + r, coefficient
// c = (first + r) % N of GLWE (first + r) / N, and word j = q N + i (q < k) of the row is
//     A_q[c - i]  for i <= c,      -A_q[N + c - i]  for i > c,        word k N = B[c].
// With j = k N the same expression reads q = k, i = 0: polynomial k is the body and 0 <= c never wraps, so the body needs
// no case of its own.  The blind-rotation kernels do this at c = 0 only, fused into their tails.
// Pure data movement, write-bound: 8 (kN + 1) bytes out per row against 8 (k + 1) N bytes per GLWE, which the N rows of one
// GLWE re-read from L2.
// Memory shape (compact_expand_kernel's): row r starts at byte 8 (kN + 1) r past the buffer, so every other row is 16-byte
// aligned and the rest are off by one word (o = 1).  A row is written as kN / 2 aligned 16-byte pairs -- words
// (o + 2p, o + 2p + 1) -- plus the one word the pairs leave out: the body (o = 0) or mask word 0 (o = 1, whose last pair is
// mask word kN - 1 and the body).  Consecutive lanes store consecutive pairs (1 KiB per wave instruction) and read
// consecutive 8-byte words downwards (the index wraps once per polynomial); a pair may straddle polynomials q, q + 1: the
// per-word function takes q from the word's own index.  The sign is a select on i > c, no branch.
// One 256-thread workgroup writes up to GLWE_EXTRACT_PAIRS_PER_WG pairs of a row, so a few dozen rows fill the GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe {

constexpr uint32_t GLWE_EXTRACT_PAIRS_PER_WG = 2048;   // 32 KB of a row per workgroup, 8 pairs per thread

struct alignas(16) GlweExtractPair {
    uint64_t lo, hi;
};

// word j of the row (j <= k N) at coefficient c of one GLWE; N a power of two
__device__ __forceinline__ uint64_t glwe_row_word(const uint64_t* __restrict__ glwe, uint32_t N, uint32_t c, uint32_t j) {
    const uint32_t i = j & (N - 1);
    const uint64_t v = glwe[(j - i) + ((c - i) & (N - 1))];   // polynomial j / N, coefficient c - i mod N: below (k + 1) N
    return i > c ? 0 - v : v;
}

// glwes = [.][k+1][N], out = [count][kN + 1]; N a power of two, kN even.
// grid = count * chunks workgroups, chunks = ceil(kN / 2 / GLWE_EXTRACT_PAIRS_PER_WG).
__global__ void __launch_bounds__(256) glwe_sample_extract_kernel(const uint64_t* __restrict__ glwes, uint64_t* __restrict__ out, uint32_t N,
                                                                  uint32_t kN, uint32_t first, uint32_t count, uint32_t chunks) {
    const uint32_t row = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (row >= count) return;
    const uint64_t block = (uint64_t)first + row;
    const uint32_t c = (uint32_t)(block & (N - 1));
    const uint64_t* __restrict__ glwe = glwes + (size_t)(block / N) * ((size_t)kN + N);
    uint64_t* __restrict__ dst = out + (size_t)row * ((size_t)kN + 1);
    const uint32_t o = (uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 3) & 1;   // words to the next 16-byte boundary
    const uint32_t pairs = kN / 2;
    const uint32_t p_lo = chunk * GLWE_EXTRACT_PAIRS_PER_WG;
    const uint32_t p_hi = p_lo + GLWE_EXTRACT_PAIRS_PER_WG < pairs ? p_lo + GLWE_EXTRACT_PAIRS_PER_WG : pairs;
#pragma unroll 4
    for (uint32_t q = p_lo + threadIdx.x; q < p_hi; q += 256) {
        const uint32_t j = o + 2 * q;                          // j + 1 <= kN
        GlweExtractPair w;
        w.lo = glwe_row_word(glwe, N, c, j);
        w.hi = glwe_row_word(glwe, N, c, j + 1);
        *reinterpret_cast<GlweExtractPair*>(dst + j) = w;      // 16-byte aligned by the choice of o
    }
    if (chunk == 0 && threadIdx.x == 0) {
        const uint32_t j = o ? 0 : kN;
        dst[j] = glwe_row_word(glwe, N, c, j);
    }
}

}  // namespace fhe
