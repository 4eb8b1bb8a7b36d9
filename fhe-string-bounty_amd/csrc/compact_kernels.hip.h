// compact_kernels.hip.h -- a public-key client's LweCompactCiphertextList expanded on the device
// (core_crypto/algorithms/lwe_compact_ciphertext_list_expansion.rs:12-58): the list holds one mask of n words per
// bin of up to n ciphertexts and one body word each; ciphertext i (bin i / n, position c = i mod n) is the bin's
// mask times X^d in Z[X]/(X^n + 1), d = n - (c + 1), then the body:
//   out[j] = A[j - d] for j >= d,  -A[n + j - d] for j < d   (0 <= j < n),   out[n] = body[i].
// A 256-char string under PARAM_MESSAGE_2_CARRY_2 arrives as 24.6 KB instead of 16.8 MB; the 16.8 MB are written
// here, in HBM.  Pure data movement, write-bound: 8 (n + 1) bytes out per row against 8 n bytes of mask per BIN,
// which every row after the bin's first finds in L2.
// Memory shape: row i starts at byte 8 (n + 1) i, so every other row is 16-byte aligned and the rest are off by one
// word (o = 1).  A row is therefore written as n / 2 aligned 16-byte pairs -- words (o + 2q, o + 2q + 1) -- plus
// the one word the pairs leave out: the body (o = 0) or mask word 0 (o = 1, whose last pair is mask word n - 1 and
// the body).  Consecutive lanes store consecutive pairs (1 KiB per wave instruction) and read consecutive 8-byte
// mask words (the rotation only moves the start and wraps once); the sign is a select on j < d, no branch.
// One 256-thread workgroup writes up to COMPACT_PAIRS_PER_WG pairs of a row: one workgroup per row up to n = 4096,
// n / 4096 of them beyond (PARAM_MESSAGE_4_CARRY_4: 8 per 256 KB row), so a list of a few dozen rows fills the GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe {

constexpr uint32_t COMPACT_PAIRS_PER_WG = 2048;   // 32 KB of a row per workgroup, 8 pairs per thread

struct alignas(16) CompactPair {
    uint64_t lo, hi;
};

// word j of the row (j <= n): the rotated, sign-folded mask, or the body at j == n
__device__ __forceinline__ uint64_t compact_row_word(const uint64_t* __restrict__ mask, uint64_t body, uint32_t n, uint32_t d, uint32_t j) {
    const uint64_t v = mask[(j - d) & (n - 1)];    // j == n reads mask[(n - d) & (n - 1)]: in bounds, value unused
    const uint64_t m = j < d ? 0 - v : v;
    return j == n ? body : m;
}

// list = [ceil(count / n)][n] masks, then [count] bodies; out = [count][n + 1]; n a power of two >= 2.
// grid = count * chunks workgroups, chunks = ceil(n / 2 / COMPACT_PAIRS_PER_WG).
__global__ void __launch_bounds__(256) compact_expand_kernel(const uint64_t* __restrict__ list, uint64_t* __restrict__ out, uint32_t n,
                                                             uint32_t count, uint32_t chunks) {
    const uint32_t row = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (row >= count) return;
    const uint32_t bins = (count + n - 1) / n;
    const uint32_t c = row & (n - 1), d = n - (c + 1);
    const uint64_t* __restrict__ mask = list + (size_t)(row / n) * n;
    const uint64_t body = list[(size_t)bins * n + row];
    uint64_t* __restrict__ dst = out + (size_t)row * (n + 1);
    const uint32_t o = (uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 3) & 1;   // words to the next 16-byte boundary
    const uint32_t pairs = n / 2;
    const uint32_t q_lo = chunk * COMPACT_PAIRS_PER_WG;
    const uint32_t q_hi = q_lo + COMPACT_PAIRS_PER_WG < pairs ? q_lo + COMPACT_PAIRS_PER_WG : pairs;
#pragma unroll 4
    for (uint32_t q = q_lo + threadIdx.x; q < q_hi; q += 256) {
        const uint32_t j = o + 2 * q;                          // j + 1 <= n
        CompactPair w;
        w.lo = compact_row_word(mask, body, n, d, j);
        w.hi = compact_row_word(mask, body, n, d, j + 1);
        *reinterpret_cast<CompactPair*>(dst + j) = w;          // 16-byte aligned by the choice of o
    }
    if (chunk == 0 && threadIdx.x == 0) {
        const uint32_t j = o ? 0 : n;
        dst[j] = compact_row_word(mask, body, n, d, j);
    }
}

}  // namespace fhe
