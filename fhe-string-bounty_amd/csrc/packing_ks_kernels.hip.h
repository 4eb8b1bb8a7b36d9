// packing_ks_kernels.hip.h -- the packing keyswitch: up to N big-key LWEs into one GLWE ciphertext, on the matrix cores.
//
// Replaces keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext
// (core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187,297-380) for whole batches.  For LWE number d of a group,
//     T_d[p][c]   = [p == k and c == 0] * body_d - sum_{i, lv} digit(a_i, lv) * PKSK[i][lv][p][c]      (mod 2^64)
//     out[p][:]  += X^d * T_d[p][:]                                             in Z[X] / (X^N + 1)
// The sum is the exact int8 matrix product of ks_mfma_kernels.hip.h with (k+1) N output columns: the digits come from
// ks_decompose_kernel (in_dim = k N), the key planes from ksk_repack_mfma_kernel (out_size = (k+1) N), the main loop
// below is keyswitch_mfma_kernel's.  Only the epilogue differs: it rotates and sums.
//
// Epilogue geometry.  N is a multiple of 32, so a 32-column group lies inside one polynomial (first coefficient c0) and
// a 32-row tile inside one GLWE (first degree d0).  Result (row r, column c) of a tile belongs at coefficient
// c0 + d0 + r + c: the 1024 results land on 63 targets, one per anti-diagonal, and the sign of a target is fixed (the
// wrap at N is the same along an anti-diagonal).  Every wave recombines its eight planes to u64 in registers, sums its
// anti-diagonals in LDS (64-bit LDS adds), and issues at most 63 global 64-bit atomic adds per (tile, K chunk).  The
// body of LWE d is T_d[k][0]: it joins anti-diagonal r of the column group that starts polynomial k, in the chunk
// blockIdx.z == 0.  Wrapping addition commutes: the result is bit-exact whatever the order.
#pragma once
#include "ks_mfma_kernels.hip.h"

namespace fhe {

struct PackKsArgs {
    const uint64_t* lwe_in;     // [count][k N + 1]; bodies are added here
    const int8_t* key;          // ksk_repack_mfma_kernel output, out_size = (k+1) N
    const int8_t* digits;       // ks_decompose_kernel output
    uint64_t* glwe_out;         // [ceil(count / N)][k+1][N], zero-filled before the launch
    KsMfmaGeom g;               // in_dim = k N, out_size = (k+1) N
    uint32_t count, row_tiles, steps_per_chunk;
    uint32_t poly_size;         // N, a multiple of 32
    uint32_t body_group;        // column group that starts polynomial k: k N / 32
};

// MT waves per workgroup = MT row tiles (32 LWEs each); grid (column groups, ceil(row tiles / MT), K chunks).
// KEEP IN STEP: the staging pipeline and the MFMA loop (down to the last __syncthreads) are keyswitch_mfma_kernel's, copied
// so that that kernel's generated code stays as it is; a change to one belongs in the other too.
template <int MT>
__global__ void __launch_bounds__(64 * MT) packing_ks_mfma_kernel(PackKsArgs a) {
    constexpr int NT = 64 * MT;
    __shared__ __align__(16) int8_t bbuf[2][8 * 1024];
    __shared__ unsigned long long diag[MT][64];             // anti-diagonal sums of every wave's tile (63 used)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cg = blockIdx.x, rt = blockIdx.y * MT + wave;
    const uint32_t s0 = blockIdx.z * a.steps_per_chunk;
    const uint32_t s1 = min(s0 + a.steps_per_chunk, a.g.steps);
    const bool active = rt < a.row_tiles;                   // waves past the batch only help staging the key
    const int8_t* kbase = a.key + ((size_t)cg * a.g.steps) * 8 * 1024;
    ksm_v16i acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0;
    diag[wave][lane] = 0;                                   // ordered before the epilogue by the barriers of the loop below

    constexpr int PER_THREAD = 8 * 1024 / 16 / NT;          // 16-byte pieces of a key tile per thread
    constexpr int DEPTH = PER_THREAD >= 4 ? 2 : 4;          // key tiles in flight per workgroup (registers) behind the LDS pair
    ksm_v4i stage[DEPTH][PER_THREAD];
    ksm_v4i afrag[DEPTH];
    const int8_t* abase = a.digits + ((size_t)(active ? rt : 0) * a.g.steps * 64 + lane) * 16;
    auto fetch = [&](uint32_t step, int slot) {
        const ksm_v4i* src = reinterpret_cast<const ksm_v4i*>(kbase + (size_t)step * 8 * 1024);
#pragma unroll
        for (int q = 0; q < PER_THREAD; q++) stage[slot][q] = src[q * NT + tid];
        afrag[slot] = *reinterpret_cast<const ksm_v4i*>(abase + (size_t)step * 1024);
    };
    auto deposit = [&](int buf, int slot) {
        ksm_v4i* dstv = reinterpret_cast<ksm_v4i*>(bbuf[buf]);
#pragma unroll
        for (int q = 0; q < PER_THREAD; q++) dstv[q * NT + tid] = stage[slot][q];
    };
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if (s0 + d < s1) fetch(s0 + d, d);
    if (s0 < s1) deposit(0, 0);
    __syncthreads();
    int cur = 0;
    for (uint32_t base = s0; base < s1; base += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const uint32_t step = base + d;
            if (step >= s1) break;
            const ksm_v4i av = afrag[d];
            if (step + DEPTH < s1) fetch(step + DEPTH, d);
            const ksm_v4i* bl = reinterpret_cast<const ksm_v4i*>(bbuf[cur]);
#pragma unroll
            for (int t = 0; t < 8; t++) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bl[t * 64 + lane], acc[t], 0, 0, 0);
            if (step + 1 < s1) deposit(cur ^ 1, (d + 1) % DEPTH);
            __syncthreads();
            cur ^= 1;
        }
    }
    if (!active) return;                                    // no workgroup barrier below: the rest is per wave
    // C layout of the 32x32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t c = lane & 31;
    unsigned long long* dg = diag[wave];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (rt * 32 + row >= a.count) continue;             // rows past the batch hold stale digits
        uint64_t p = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) p += (uint64_t)(int64_t)acc[t][r] << (8 * t);
        atomicAdd(&dg[row + c], (unsigned long long)(0 - p));
    }
    // the body of LWE d is T_d[k][0]: column 0 of polynomial k, anti-diagonal = its row
    if (blockIdx.z == 0 && cg == a.body_group && lane < 32 && rt * 32 + lane < a.count)
        atomicAdd(&dg[lane], (unsigned long long)a.lwe_in[(size_t)(rt * 32 + lane) * (a.g.in_dim + 1) + a.g.in_dim]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane >= 63) return;
    const uint32_t N = a.poly_size;
    const uint32_t first = rt * 32, glwe = first / N, d0 = first % N;
    const uint32_t poly = cg * 32 / N, c0 = cg * 32 % N;
    uint32_t pos = c0 + d0 + lane;                          // < 2 N - 1
    uint64_t v = dg[lane];
    if (pos >= N) { pos -= N; v = 0 - v; }                  // X^N = -1
    atomicAdd(reinterpret_cast<unsigned long long*>(a.glwe_out + ((size_t)glwe * (a.g.out_size / N) + poly) * N + pos), (unsigned long long)v);
}

}  // namespace fhe
