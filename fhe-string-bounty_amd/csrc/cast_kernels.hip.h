// cast_kernels.hip.h -- the casting keys' own kernel: the matrix-core keyswitch's digit fragments straight from packed GLWEs.
//
// A stored string is a few packed GLWEs of the source client (block b = coefficient c_b = (first + b) % N of GLWE
// (first + b) / N).  The GLWE key flattened is the big LWE key, so block b IS the LWE
//     mask[q N + i] = A_q[c_b - i] for i <= c_b,  -A_q[N + c_b - i] for i > c_b        (q < k),        body = B[c_b]
// (glwe_extract_kernels.hip.h) and casting it needs only the signed digits of those mask words in the A-fragment layout
// ks_decompose_kernel writes (ks_mfma_prep_kernels.hip.h):
//     digits[row tile = b / 32][step][lane = h * 32 + b % 32][16],   slot group 2 step + h = epg whole mask elements.
// cast_decompose_glwe_kernel computes every word from the GLWE, decomposes it and stores the fragment: the extracted LWE
// is never written -- 8 (k N + 1) bytes per block, 16.8 MB for the 1,024 blocks of a 256-character
// PARAM_MESSAGE_2_CARRY_2 string, written and read again otherwise -- and the bodies B[c_b] go to a dense array that the
// product reads with stride 1 (KsMfmaArgs::bodies).
//
// Shape: one wave per (row tile, step), four waves per workgroup.  Lane (h, r) holds row b = 32 tile + r and slot group
// 2 step + h, so the wave's 64 fragments are the 1 KiB that (tile, step) owns: ONE coalesced 16-byte store per lane.
// Reads: consecutive rows sit at consecutive coefficients, so for a fixed element the 32 lanes of a half read 32
// consecutive words of one polynomial (the index wraps once per N, and once more where the batch crosses into the next
// GLWE); a GLWE's (k + 1) N words are re-read by its N rows from L2.  The sign of the wrapped part is a select, the
// position of a digit inside the fragment is a compile-time slot (no dynamically indexed private array).  Rows past the
// batch store nothing: their fragments keep what the buffer held, as with ks_decompose_kernel, and the product drops
// their sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ks_mfma_kernels.hip.h"

namespace fhe {

struct CastDecomposeArgs {
    const uint64_t* glwes;      // [.][k+1][N] of the SOURCE parameter set, from the GLWE that holds block 0
    int8_t* digits;             // [row tile][step][64][16]
    uint64_t* bodies;           // [batch]
    KsMfmaGeom g;               // in_dim = k N
    uint32_t N, first, batch, row_tiles;
};

constexpr int CAST_DECOMPOSE_WAVES = 4;

// grid (ceil(steps / CAST_DECOMPOSE_WAVES), row tiles), 64 * CAST_DECOMPOSE_WAVES threads; N a power of two
__global__ void __launch_bounds__(64 * CAST_DECOMPOSE_WAVES) cast_decompose_glwe_kernel(CastDecomposeArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t step = blockIdx.x * CAST_DECOMPOSE_WAVES + wave, rt = blockIdx.y;
    if (step >= a.g.steps || rt >= a.row_tiles) return;
    const uint32_t h = lane >> 5, b = rt * 32 + (lane & 31);
    if (b >= a.batch) return;
    const uint32_t N = a.N, in_dim = a.g.in_dim;
    const uint64_t block = (uint64_t)a.first + b;
    const uint32_t c = (uint32_t)(block & (N - 1));
    const uint64_t* __restrict__ glwe = a.glwes + (size_t)(block / N) * ((size_t)in_dim + N);
    if (step == 0 && h == 0) a.bodies[b] = glwe[(size_t)in_dim + c];
    const uint32_t L = a.g.level, bl = a.g.base_log, rep = bl * L;
    const uint64_t mask = (1ull << bl) - 1;
    int8_t frag[16];
#pragma unroll
    for (int j = 0; j < 16; j++) frag[j] = 0;
    for (uint32_t e = 0; e < a.g.epg; e++) {
        const uint32_t j = (2 * step + h) * a.g.epg + e;         // mask word of the row; the pad elements past k N are zero
        uint64_t x = 0;
        if (j < in_dim) {
            const uint32_t i = j & (N - 1);
            const uint64_t v = glwe[(j - i) + ((c - i) & (N - 1))];   // polynomial j / N, coefficient c - i mod N: below k N
            x = i > c ? 0 - v : v;
        }
        // the reference's signed decomposition, level L first (iter.rs:101-127): ks_decompose_kernel's, word for word
        const uint64_t t = x >> (63 - rep);
        uint64_t state = ((t + 1) >> 1) & ((1ull << rep) - 1);
        for (uint32_t lv = 0; lv < L; lv++) {
            uint64_t res = state & mask;
            state >>= bl;
            uint64_t carry = ((res - 1ull) | state) & res;
            carry >>= bl - 1;
            state += carry;
            const int8_t d = (int8_t)((int32_t)(uint32_t)res - (int32_t)((uint32_t)carry << bl));
#pragma unroll
            for (int s = 0; s < 16; s++) frag[s] = (uint32_t)s == e * L + lv ? d : frag[s];
        }
    }
    ksm_v4i w;
    __builtin_memcpy(&w, frag, 16);
    *reinterpret_cast<ksm_v4i*>(a.digits + (((size_t)rt * a.g.steps + step) * 64 + lane) * 16) = w;
}

}  // namespace fhe
