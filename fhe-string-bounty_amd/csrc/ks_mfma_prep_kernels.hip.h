// ks_mfma_prep_kernels.hip.h -- the two kernels that prepare the operands of the matrix-core products of ks_mfma_kernels.hip.h
// and packing_ks_kernels.hip.h: the key's digit planes (once per key) and a batch's digit fragments (once per launch).
// They are not templates, so exactly one translation unit may include this file: engine.hip, which launches them for both
// products through ks_mfma_repack and ks_mfma_digits (ks_mfma_launch.h).
#pragma once
#include "ks_mfma_kernels.hip.h"

namespace fhe {

// Key words -> balanced base-256 digit planes in B-fragment order.  One thread per (column group, step, lane, plane-octet).
__global__ void __launch_bounds__(64) ksk_repack_mfma_kernel(const uint64_t* __restrict__ ksk, int8_t* __restrict__ out, KsMfmaGeom g,
                                                             uint32_t first_step) {
    const uint32_t cg = blockIdx.x, step = first_step + blockIdx.y, lane = threadIdx.x;   // a launch covers one span of the steps (grid_spans.h)
    const uint32_t c = lane & 31, h = lane >> 5;
    const uint32_t col = cg * 32 + c;
    int8_t frag[8][16];
#pragma unroll
    for (int t = 0; t < 8; t++)
#pragma unroll
        for (int j = 0; j < 16; j++) frag[t][j] = 0;
    for (uint32_t j = 0; j < g.epg * g.level; j++) {
        const uint32_t i = (step * 2 + h) * g.epg + j / g.level, lv = j % g.level;
        uint64_t k = 0;
        if (i < g.in_dim && col < g.out_size) k = ksk[((size_t)i * g.level + lv) * g.out_size + col];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int8_t s = (int8_t)(uint8_t)(k & 0xff);        // balanced digit: low byte read as signed
            frag[t][j] = s;
            k = (k - (uint64_t)(int64_t)s) >> 8;                  // exact: k - s is a multiple of 256 (mod 2^64)
        }
    }
    int8_t* dst = out + (((size_t)cg * g.steps + step) * 8) * 1024 + (size_t)lane * 16;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        ksm_v4i w;
        __builtin_memcpy(&w, frag[t], 16);
        *reinterpret_cast<ksm_v4i*>(dst + (size_t)t * 1024) = w;
    }
}

// One thread per (sample, 16-slot group): the reference's signed decomposition (level L first, iter.rs:101-127) of the
// group's floor(16 / level) mask elements, stored as ONE 16-byte A-fragment element (pad slots written as zero digits).
__global__ void __launch_bounds__(256) ks_decompose_kernel(KsDecomposeArgs a) {
    const uint32_t grp = blockIdx.x * 256 + threadIdx.x, b = a.first + blockIdx.y;   // a launch covers one span of the batch (grid_spans.h)
    if (grp >= 2 * a.g.steps || b >= a.batch) return;
    const uint32_t L = a.g.level, bl = a.g.base_log, rep = bl * L;
    const uint64_t mask = (1ull << bl) - 1;
    const uint64_t* src = a.lwe_in + (size_t)b * (a.g.in_dim + 1);
    int8_t frag[16];
#pragma unroll
    for (int j = 0; j < 16; j++) frag[j] = 0;
    for (uint32_t e = 0; e < a.g.epg; e++) {
        const uint32_t i = grp * a.g.epg + e;
        const uint64_t x = i < a.g.in_dim ? src[i] : 0;
        const uint64_t t = x >> (63 - rep);
        uint64_t state = ((t + 1) >> 1) & ((1ull << rep) - 1);
        for (uint32_t lv = 0; lv < L; lv++) {
            uint64_t res = state & mask;
            state >>= bl;
            uint64_t carry = ((res - 1ull) | state) & res;
            carry >>= bl - 1;
            state += carry;
            const int8_t d = (int8_t)((int32_t)(uint32_t)res - (int32_t)((uint32_t)carry << bl));
            // frag[e * L + lv] without a dynamically indexed private array
#pragma unroll
            for (int j = 0; j < 16; j++) frag[j] = (uint32_t)j == e * L + lv ? d : frag[j];
        }
    }
    const uint32_t step = grp >> 1, h = grp & 1;
    ksm_v4i w;
    __builtin_memcpy(&w, frag, 16);
    *reinterpret_cast<ksm_v4i*>(a.digits + (((size_t)(b >> 5) * a.g.steps + step) * 64 + (h * 32 + (b & 31))) * 16) = w;
}

}  // namespace fhe
