// ring_packing_kernels.hip.h -- ring packing on the device (ring_packing.h has the definition): the leaves, and per tree
// level a batch of independent merges in three launches,
//   ring_digits_kernel    sigma_t(e - X^s o) per merge: the digit polynomials, transformed, and the permuted body;
//   ring_mac_kernel       per (merge, output polynomial, plane): the pointwise products against the resident transformed
//                         planes summed over q and level, the inverse transform, the centred lift;
//   ring_combine_kernel   (e + X^s o) + (0, .., sigma_t(B)) - sum_plane 256^plane lift, written over e.
// Included by packing_dev.hip alone.
//
// One workgroup transforms one polynomial in LDS: N 32-bit words, 128 KB at N = 32768 (one workgroup per CU), radix-2
// passes with a barrier each.  A pass at butterfly distance t >= 32 reads and writes consecutive words from consecutive
// lanes, so no two lanes of a 32-lane half meet on a bank; in the five passes below that a half reads runs of t words out
// of every 2 t, 32 words spread over a span of 64: two per bank, a 2-way conflict, which this first version pays.
// Slots: slot j of the scratch is leaf j; the node (l, r) of group g lives in slot g N + r, which its even child held.  A
// merge reads slots g N + r and g N + r + s and writes the first: merges of one level never touch each other's slots, and
// ring_combine_kernel reads each word of e only in the thread that writes it.  Vector stores only, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "ring_packing.h"

namespace fhe {

constexpr uint32_t RING_THREADS_MAX = 1024;

// One tree level's batch of merges: merge m of the level is node r of group g -- every full group has min(s, N) = s merges,
// the last, ragged one min(s, c_last).
struct RingLevelArgs {
    uint64_t* slots;              // count x [k+1][N]
    uint32_t* digits;             // batch x [k L][N], transformed
    uint64_t* sigma_b;            // batch x [N]
    int32_t* lifted;              // batch x [k+1][8][N]
    const uint32_t* key;          // this level's planes [k L][k+1][8][N], transformed
    const uint32_t *fwd, *inv;    // twiddles
    uint64_t* final_out;          // the last level writes GLWE g here instead of over e; else null
    uint32_t N, logN, k, L, base_log, n_inv;
    uint32_t s, tinv, full_groups, c_last, first;   // first: the batch's first merge
};

struct RingMerge {
    uint64_t* e;
    const uint64_t* o;            // null: the odd child holds no leaf
    uint32_t group;
};

__device__ inline RingMerge ring_merge_of(const RingLevelArgs& a, uint32_t local) {
    const uint32_t m = a.first + local, full = a.full_groups * a.s;
    const uint32_t g = m < full ? m / a.s : a.full_groups, r = m < full ? m % a.s : m - full;
    const uint32_t c_g = g < a.full_groups ? a.N : a.c_last;
    const size_t glwe_len = (size_t)(a.k + 1) * a.N;
    RingMerge out;
    out.e = a.slots + ((size_t)g * a.N + r) * glwe_len;
    out.o = r + a.s < c_g ? a.slots + ((size_t)g * a.N + r + a.s) * glwe_len : nullptr;
    out.group = g;
    return out;
}

// In place in LDS; every thread of the workgroup calls it, the data visible (a barrier behind the last write) on entry and on exit.
__device__ inline void ring_ntt_forward_lds(uint32_t* a, uint32_t N, uint32_t logN, const uint32_t* __restrict__ fwd) {
    uint32_t lt = logN;
    for (uint32_t m = 1; m < N; m <<= 1) {
        lt--;
        const uint32_t t = 1u << lt;
        for (uint32_t b = threadIdx.x; b < N / 2; b += blockDim.x) {
            const uint32_t i = b >> lt, j = (i << (lt + 1)) + (b & (t - 1));
            const uint32_t U = a[j], V = ring_mul(a[j + t], fwd[m + i]);
            a[j] = ring_add(U, V);
            a[j + t] = ring_sub(U, V);
        }
        __syncthreads();
    }
}

// The scaling by N^-1 is left to the caller.
__device__ inline void ring_ntt_inverse_lds(uint32_t* a, uint32_t N, const uint32_t* __restrict__ inv) {
    uint32_t lt = 0;
    for (uint32_t m = N; m > 1; m >>= 1, lt++) {
        const uint32_t t = 1u << lt, h = m >> 1;
        for (uint32_t b = threadIdx.x; b < N / 2; b += blockDim.x) {
            const uint32_t i = b >> lt, j = (i << (lt + 1)) + (b & (t - 1));
            const uint32_t U = a[j], V = a[j + t];
            a[j] = ring_add(U, V);
            a[j + t] = ring_mul(ring_sub(U, V), inv[h + i]);
        }
        __syncthreads();
    }
}

// count polynomials of N residues at `polys`, transformed in place: the transform on its own (fhe_engine_ring_ntt).
__global__ void __launch_bounds__(RING_THREADS_MAX) ring_ntt_kernel(uint32_t* __restrict__ polys, const uint32_t* __restrict__ fwd, const uint32_t* __restrict__ inv,
                                                                    uint32_t N, uint32_t logN, uint32_t n_inv, int inverse) {
    extern __shared__ uint32_t ring_lds[];
    uint32_t* poly = polys + (size_t)blockIdx.x * N;
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) ring_lds[i] = poly[i];
    __syncthreads();
    if (inverse) ring_ntt_inverse_lds(ring_lds, N, inv); else ring_ntt_forward_lds(ring_lds, N, logN, fwd);
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) poly[i] = inverse ? ring_mul(ring_lds[i], n_inv) : ring_lds[i];
}

// The resident key: row (tree level, q, it, output polynomial) of the 64-bit key x plane -> the transformed plane.
// grid (rows, 8).
__global__ void __launch_bounds__(RING_THREADS_MAX) ring_key_planes_kernel(const uint64_t* __restrict__ key, uint32_t* __restrict__ planes, const uint32_t* __restrict__ fwd,
                                                                           uint32_t N, uint32_t logN) {
    extern __shared__ uint32_t ring_lds[];
    const uint64_t* src = key + (size_t)blockIdx.x * N;
    uint32_t* dst = planes + ((size_t)blockIdx.x * RING_PLANES + blockIdx.y) * N;
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) ring_lds[i] = ring_from_signed(ring_plane(src[i], blockIdx.y));
    __syncthreads();
    ring_ntt_forward_lds(ring_lds, N, logN, fwd);
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) dst[i] = ring_lds[i];
}

// One thread per word of a leaf: grid (ceil((k+1) N / 256), count).
__global__ void __launch_bounds__(256) ring_leaf_kernel(const uint64_t* __restrict__ cts, uint64_t* __restrict__ slots, uint32_t N, uint32_t logN, uint32_t k) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= (k + 1) * N) return;
    const uint64_t* ct = cts + (size_t)blockIdx.y * ((size_t)k * N + 1);
    const uint32_t q = w >> logN, i = w & (N - 1);
    uint64_t v = 0;
    if (q < k) v = i ? 0 - ring_leaf_word(ct[q * N + N - i], logN) : ring_leaf_word(ct[q * N], logN);
    else if (i == 0) v = ring_leaf_word(ct[k * N], logN);
    slots[(size_t)blockIdx.y * ((size_t)(k + 1) * N) + w] = v;
}

// grid (merges of the batch, k L + 1).  y < k L: digit polynomial (q, it) of sigma_t(e - X^s o), transformed; y = k L: the
// permuted body sigma_t(B_e - X^s B_o), which ring_combine_kernel adds -- gathered here, while nobody writes e.
__global__ void __launch_bounds__(RING_THREADS_MAX) ring_digits_kernel(RingLevelArgs a) {
    extern __shared__ uint32_t ring_lds[];
    const RingMerge mg = ring_merge_of(a, blockIdx.x);
    const uint32_t N = a.N, kL = a.k * a.L, y = blockIdx.y;
    const uint32_t q = y < kL ? y / a.L : a.k, it = y < kL ? y % a.L : 0;
    const uint64_t* eq = mg.e + (size_t)q * N;
    const uint64_t* oq = mg.o ? mg.o + (size_t)q * N : nullptr;
    for (uint32_t c = threadIdx.x; c < N; c += blockDim.x) {
        bool neg;
        const uint32_t j = ring_auto_source(N, a.tinv, c, &neg);
        uint64_t v = eq[j];
        if (oq) v -= ring_shifted(oq, N, a.s, j);
        if (neg) v = 0 - v;
        if (y < kL) ring_lds[c] = ring_from_signed(ring_digit(v, a.base_log, a.L, it));
        else a.sigma_b[(size_t)blockIdx.x * N + c] = v;
    }
    if (y == kL) return;                      // the whole workgroup: no barrier is left waiting
    __syncthreads();
    ring_ntt_forward_lds(ring_lds, N, a.logN, a.fwd);
    uint32_t* dst = a.digits + ((size_t)blockIdx.x * kL + y) * N;
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) dst[i] = ring_lds[i];
}

// grid (merges of the batch, (k+1) 8): y = output polynomial x 8 + plane.
__global__ void __launch_bounds__(RING_THREADS_MAX) ring_mac_kernel(RingLevelArgs a) {
    extern __shared__ uint32_t ring_lds[];
    const uint32_t N = a.N, kL = a.k * a.L, k1 = a.k + 1;
    const uint32_t* d = a.digits + (size_t)blockIdx.x * kL * N;
    const uint32_t* key = a.key + (size_t)blockIdx.y * N;           // + x (k+1) 8 N per term
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) {
        uint64_t sum = 0;                                           // at most 128 terms below 2^32 each
        for (uint32_t x = 0; x < kL; x++) sum += ring_mul(d[(size_t)x * N + i], key[(size_t)x * k1 * RING_PLANES * N + i]);
        ring_lds[i] = ring_reduce(sum);
    }
    __syncthreads();
    ring_ntt_inverse_lds(ring_lds, N, a.inv);
    int32_t* dst = a.lifted + ((size_t)blockIdx.x * k1 * RING_PLANES + blockIdx.y) * N;
    for (uint32_t c = threadIdx.x; c < N; c += blockDim.x) dst[c] = (int32_t)ring_lift(ring_mul(ring_lds[c], a.n_inv));
}

// One thread per coefficient of an output polynomial: grid (ceil(N / 256), k + 1, merges of the batch).
__global__ void __launch_bounds__(256) ring_combine_kernel(RingLevelArgs a) {
    const uint32_t N = a.N, c = blockIdx.x * 256 + threadIdx.x, qo = blockIdx.y, k1 = a.k + 1;
    if (c >= N) return;
    const RingMerge mg = ring_merge_of(a, blockIdx.z);
    const int32_t* lifted = a.lifted + ((size_t)blockIdx.z * k1 + qo) * RING_PLANES * N;
    uint64_t prod = 0;
#pragma unroll
    for (uint32_t pl = 0; pl < RING_PLANES; pl++) prod += (uint64_t)(int64_t)lifted[(size_t)pl * N + c] << (8 * pl);
    uint64_t v = mg.e[(size_t)qo * N + c] - prod;
    if (mg.o) v += ring_shifted(mg.o + (size_t)qo * N, N, a.s, c);
    if (qo == a.k) v += a.sigma_b[(size_t)blockIdx.z * N + c];
    uint64_t* dst = a.final_out ? a.final_out + (size_t)mg.group * k1 * N : mg.e;
    dst[(size_t)qo * N + c] = v;
}

}  // namespace fhe
