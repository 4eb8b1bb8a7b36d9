// transcipher_kernels.hip.h -- the Trivium / Kreyvium round on the device (the definition: transcipher.h; the host
// restatement the kernels are compared with word for word: transcipher.cpp).
//
// All three kernels build one output row per workgroup as a sum of at most TC_MAX_SRC rows mod 2^64 (tc_sum_rows): the
// state taps of a lookup input, the `bits` keystream lookups of a string block, or one key row copied into the initial
// state.  Which rows, and the multiplier of the two ANDed taps, come from (cipher, row, round) by the arithmetic of
// tc_sources / tc_ring_row: no recipe table in memory.  No LDS, no atomics.
//
// Loads and stores are 16-byte pairs.  A row has kN + 1 words, an odd number, so rows alternate between starting on a
// 16-byte boundary and 8 bytes past one.  The destination decides the pairing, as in glwe_extract_kernels.hip.h: with
// o = words to its next boundary, thread q owns words (o + 2 q, o + 2 q + 1), q < kN / 2, and the one word the pairs leave
// out (word 0 if o = 1, else the body, word kN) is summed once by thread 0, which also stores the row's table index.  A
// source row of the same parity is read at the same pairing.  A source of the other parity is read at ITS aligned pairs
// and the word a thread lacks comes from the neighbouring lane's pair by a wave shuffle; only the lane at the wave's
// edge (and the thread that owns the row's last pair) loads that one word by itself.  Every load stays inside its row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "transcipher.h"

namespace fhe {

struct alignas(16) TcPair { uint64_t lo, hi; };

__device__ __forceinline__ uint32_t tc_parity(const uint64_t* p) { return (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 3) & 1; }
// Every row lies in device memory (hipMalloc): saying so keeps the loads global ones where the compiler, after the rows'
// addresses went through an array, would issue flat loads.
typedef uint64_t TcVec2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ TcPair tc_pair_at(const uint64_t* p) {
    const TcVec2 v = *(const __attribute__((address_space(1))) TcVec2*)p;      // 16-byte aligned by the callers
    return TcPair{v.x, v.y};
}
__device__ __forceinline__ uint64_t tc_word_at(const uint64_t* p) { return *(const __attribute__((address_space(1))) uint64_t*)p; }

// words (o + 2 q, o + 2 q + 1) of the row at src, q < pairs = kN / 2.  src and o are uniform over the workgroup; the lanes
// of a wave hold consecutive q and the active ones are a prefix of the wave (the callers' strided loops).
__device__ __forceinline__ TcPair tc_load_pair(const uint64_t* __restrict__ src, uint32_t o, uint32_t q, uint32_t pairs) {
    const uint64_t* at = src + o + 2 * q;
    if (tc_parity(src) == o) return tc_pair_at(at);
    const uint32_t lane = threadIdx.x & 63;
    TcPair w;
    if (o == 0) {                                                       // aligned pairs start at odd words: (2 q + 1, 2 q + 2), 2 q + 2 <= kN
        const TcPair p = tc_pair_at(at + 1);
        w.lo = __shfl_up((unsigned long long)p.hi, 1);                  // word 2 q: the previous lane's second
        if (lane == 0) w.lo = tc_word_at(at);
        w.hi = p.lo;
    } else {                                                            // o = 1, aligned pairs at even words: (2 q, 2 q + 1)
        const TcPair p = tc_pair_at(at - 1);
        w.hi = __shfl_down((unsigned long long)p.lo, 1);                // word 2 q + 2: the next lane's first
        if (lane == 63 || q + 1 == pairs) w.hi = tc_word_at(at + 1);                // 2 q + 2 <= kN: the body at the row's end
        w.lo = p.hi;
    }
    return w;
}

// dst[0 .. big) = mul * (src[0] + .. + src[n_and - 1]) + src[n_and] + .. + src[n - 1], mod 2^64, with `body` added to the
// last word by the one thread that stores it; n <= TC_MAX_SRC, all of it uniform over the workgroup of 256 threads.
__device__ __forceinline__ void tc_sum_rows(uint64_t* __restrict__ dst, const uint64_t* const (&src)[TC_MAX_SRC], uint32_t n, uint32_t n_and, uint64_t mul,
                                            uint32_t big, uint64_t body = 0) {
    const uint32_t o = tc_parity(dst), pairs = (big - 1) / 2;
    for (uint32_t q = threadIdx.x; q < pairs; q += 256) {
        TcPair acc{0, 0};
#pragma unroll
        for (uint32_t i = 0; i < TC_MAX_SRC; i++)
            if (i < n) {
                const TcPair w = tc_load_pair(src[i], o, q, pairs);
                const uint64_t c = i < n_and ? mul : 1;
                acc.lo += c * w.lo;
                acc.hi += c * w.hi;
            }
        if (o && q + 1 == pairs) acc.hi += body;                       // o = 1: the last pair ends in the body
        *reinterpret_cast<TcPair*>(dst + o + 2 * q) = acc;             // 16-byte aligned by the choice of o
    }
    if (threadIdx.x == 0) {
        const uint32_t j = o ? 0 : big - 1;
        uint64_t acc = o ? 0 : body;
#pragma unroll
        for (uint32_t i = 0; i < TC_MAX_SRC; i++)
            if (i < n) acc += (i < n_and ? mul : 1) * tc_word_at(src[i] + j);
        dst[j] = acc;
    }
}

struct TcDeviceShape {
    uint32_t big, bits, cipher, S;
    uint64_t delta;
};

// ring = tc_ring_rows(S) rows, key = L rows K_1 .. K_L, ivs = S x L / 8 bytes.  grid = S * 2 * 192: the blocks of rounds
// -1 and -2.  A key bit is its resident row, a clear bit a trivial ciphertext.
__global__ void __launch_bounds__(256) transcipher_init_kernel(TcDeviceShape sh, const uint64_t* __restrict__ key, const uint8_t* __restrict__ ivs,
                                                               uint64_t* __restrict__ ring) {
    const uint32_t s = blockIdx.x / (2 * TC_STATE_ROWS), at = blockIdx.x % (2 * TC_STATE_ROWS);
    if (s >= sh.S) return;
    const uint32_t reg = (at % TC_STATE_ROWS) >> 6, i = 1 + (at % TC_STATE_ROWS & 63) + 64 * (at / TC_STATE_ROWS);   // 1 .. 128
    const uint32_t L = stream_key_bits(sh.cipher);
    uint64_t* __restrict__ dst = ring + tc_ring_row(sh.S, s, reg, -(int32_t)i) * sh.big;
    const StreamInit si = stream_initial(sh.cipher, reg, i);
    const uint64_t* src[TC_MAX_SRC] = {};
    uint32_t n = 0;
    if (si.what == STREAM_INIT_KEY) src[n++] = key + (size_t)(si.j - 1) * sh.big;
    uint64_t body = 0;                                                  // a clear bit: zeros and bit * delta in the body
    if (si.what != STREAM_INIT_KEY) body = (si.what == STREAM_INIT_IV ? stream_spec_bit(ivs + (size_t)s * (L / 8), L, si.j) : si.what) * sh.delta;
    tc_sum_rows(dst, src, n, 0, 1, sh.big, body);
}

struct TcGatherArgs {
    TcDeviceShape sh;
    const uint64_t* ring;
    const uint64_t* key;
    const uint8_t* ivs;
    const uint8_t* data;                // S x n_bytes clear cipher bytes, or null (warm-up)
    uint64_t* pbs_in;                   // S x rows rows
    uint32_t* tables;                   // S x rows
    int32_t round;
    uint32_t rows, n_bytes, m;
    uint32_t lut_of[TC_MAX_TABLES];     // table number -> the engine's table index
};

// The PBS inputs and table indices of one round of S streams: grid = S * rows, one workgroup per row.
__global__ void __launch_bounds__(256) transcipher_gather_kernel(TcGatherArgs a) {
    const uint32_t s = blockIdx.x / a.rows, row = blockIdx.x % a.rows;
    if (s >= a.sh.S) return;
    const uint32_t kind = row >> 6, j = row & 63, big = a.sh.big;
    const TcSources r = tc_sources(a.sh.cipher, kind, 64 * a.round + (int32_t)j);
    const uint64_t* src[TC_MAX_SRC] = {};
    // the ANDed taps first (tc_sources' order), then the XORed state taps, then the key row
#pragma unroll
    for (uint32_t i = 0; i < 6; i++)
        if (i < r.n) src[i] = a.ring + tc_ring_row(a.sh.S, s, r.kind[i], r.step[i]) * big;
    uint32_t n = r.n;
    if (r.key_row != TC_NONE) {
        const uint64_t* k = a.key + (size_t)r.key_row * big;
        if (n == 5) src[5] = k; else src[6] = k;                        // static indices: the array stays in registers
        n++;
    }
    tc_sum_rows(a.pbs_in + (size_t)blockIdx.x * big, src, n, r.n_and, r.mul, big);
    if (threadIdx.x == 0) {
        const uint32_t L = stream_key_bits(a.sh.cipher);
        uint32_t table;
        if (kind == TC_KEYSTREAM) table = tc_keystream_table(j, a.sh.bits, tc_data_bit(a.data, a.n_bytes, s, a.m, j));
        else table = tc_state_table(r, r.iv_j != TC_NONE ? stream_spec_bit(a.ivs + (size_t)s * (L / 8), L, r.iv_j) : 0);
        a.tables[blockIdx.x] = a.lut_of[table];
    }
}

// The string blocks of one data round: block b of character ch is the sum of its `bits` keystream lookups.  grid =
// S * chars * blocks_per_char with chars = min(8, n_bytes - 8 m); out = S x n_bytes x blocks_per_char rows.
__global__ void __launch_bounds__(256) transcipher_apply_kernel(TcDeviceShape sh, const uint64_t* __restrict__ ring, uint64_t* __restrict__ out, int32_t round,
                                                                uint32_t n_bytes, uint32_t m, uint32_t chars) {
    const uint32_t bpc = 8 / sh.bits;
    const uint32_t s = blockIdx.x / (chars * bpc), c = blockIdx.x / bpc % chars, b = blockIdx.x % bpc;
    if (s >= sh.S) return;
    const uint64_t* src[TC_MAX_SRC] = {};
#pragma unroll
    for (uint32_t i = 0; i < TC_MAX_SRC; i++)
        if (i < sh.bits) src[i] = ring + tc_ring_row(sh.S, s, TC_KEYSTREAM, 64 * round + (int32_t)(8 * c + sh.bits * b + i)) * sh.big;
    tc_sum_rows(out + (((size_t)s * n_bytes + 8 * m + c) * bpc + b) * sh.big, src, sh.bits, 0, 1, sh.big);
}

}  // namespace fhe
