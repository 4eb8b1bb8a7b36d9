// blind_rotate.h -- what the host knows about the blind-rotation kernels: one descriptor per launchable kernel and the
// variant registry built from them.  Host only: no kernel header is needed to read it.  The kernels, the registry's
// contents and every launch live in blind_rotate.hip; engine.hip reads a variant's shape flags through this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fhestr.h"
#include "device_buffer.h"

namespace fhe {

struct Engine;
struct ClusterCtl;      // pbs_cluster_kernels.hip.h
struct ClusterStatus;

// A kernel and its launch shape, filled in from the kernel's own config struct where the kernel is instantiated.
struct KernelRef {
    const void* fn = nullptr;
    int threads = 0;
    size_t lds_fixed = 0;
    int lds_per_n = 0;      // dynamic LDS bytes per small-LWE coefficient (modulus-switched mask / degrees)
    explicit operator bool() const { return fn != nullptr; }
    size_t lds(uint32_t n) const { return lds_fixed + (size_t)n * lds_per_n; }
};

// The one way a descriptor is launched: its block size, its LDS for a small-LWE dimension n -- or `lds`, where a caller
// asks for more than the kernel needs (rotate_multi_cu: one workgroup per CU).
inline hipError_t launch(const KernelRef& k, dim3 grid, void** args, uint32_t n, hipStream_t stream, size_t lds = 0) {
    return hipLaunchKernel(k.fn, grid, dim3(k.threads), args, lds ? lds : k.lds(n), stream);
}

// ---- blind-rotation variant registry ----------------------------------------------------------
struct BrVariant {
    int logN, k1, L, logR;
    bool wide;          // true: every thread carries all k+1 polynomials (blind_rotate_wide_kernel)
    bool large;         // true: four-step FFT through an HBM workspace (blind_rotate_large_kernel)
    int grouping = 1;   // > 1: multi-bit PBS kernel for that grouping factor
    KernelRef rotate;
    size_t ws_bytes = 0;            // per-LWE workspace (large only)
    KernelRef rotate_keypf;         // wide layout with the whole key of a step prefetched (single launches only, see BrWideCfg)
    KernelRef convert;              // standard-domain polynomials -> this variant's Fourier layout
    size_t convert_ws = 0;          // per-workgroup workspace of the conversion kernel (large only)
    bool convert_one_per_block = false;   // the conversion kernel takes one polynomial per workgroup (K1 otherwise)
    // multi-bit, small batches: build every (LWE, group) GGSW on the whole GPU first, then rotate against them
    KernelRef combine, rotate_combined;
    int combine_grid_y = 1;         // grid (n/G, combine_grid_y, ceil(batch / combine_chunk))
    int combine_chunk = 1;
    size_t combined_bytes = 0;      // one combined GGSW
    // multi-bit on every other shape: two-kernel path only (generic combine + the classic kernel's EXTPROD mode, which is `rotate`)
    bool rotate_is_extprod = false;
    KernelRef combine_generic;
    int combine_generic_elems = 1;  // grid (n/G, ceil(GGSW elements / combine_generic_elems), ceil(batch / combine_generic_chunk))
    int combine_generic_chunk = 1;
    // N >= 16384: several compute units of one XCD per LWE (pbs_cluster_kernels.hip.h); same Fourier key as `rotate`
    KernelRef cluster;
    int cluster_size = 0;           // workgroups per LWE
    size_t cluster_ws = 0;          // workspace bytes per cluster
    // N = 32768, two levels: all CUs of an XCD per LWE, two LWEs in flight per XCD (pbs_xcd_kernels.hip.h)
    KernelRef xcd;
    int xcd_size = 0;
    size_t xcd_ws = 0, xcd_lds_one_per_cu = 0;   // an LDS request that lets a CU take only one of its workgroups
    // dense layout (pbs_dense_kernels.hip.h): four workgroups per CU, for batches beyond two LWEs per CU
    KernelRef dense;
    KernelRef dense_convert;        // its Fourier key is in its own plan's order: a second copy of the key
};

// selector: 0 = default; otherwise log2(points per thread) + 16 if the "wide" layout is wanted
const BrVariant* find_variant(const fhe_params_t& p, int selector);

// The engine's two variants for a selector: `small` up to one LWE per CU, `large` above.  Selector 0 (automatic): the "wide"
// twin of the default (same points per thread => same key layout) serves the big batches.
struct BrVariantPair { const BrVariant *small, *large; };
BrVariantPair find_variant_pair(const fhe_params_t& p, int selector);

// ---- what the multi-CU rotation paths keep between launches (the 8-CU clusters and the whole-XCD kernel) ---------------------
// One device block holds the ClusterCtl (tickets, flags: zeroed per launch) and, right behind it, the ClusterStatus (sticky
// until the host has read an error out of it).  Defined in blind_rotate.hip.
struct MultiCuRuntime {
    DeviceBuffer<unsigned char> ws;   // exchange matrices: 1.5 MB per cluster (L2-resident by design)
    DeviceBuffer<void> block;         // ClusterCtl + ClusterStatus
    bool unchecked = false;           // a launch whose status words have not been read yet (cfg.cluster_fallback off)
    uint32_t last = 0;                // clusters the last checked launch formed
    uint32_t n_fallbacks = 0;         // launches that gave up and were re-run on the one-workgroup kernel
    uint32_t last_error = 0;          // the status code of the latest of them
    int xcd_per_cu = -1;              // workgroups of the whole-XCD kernel a CU holds (occupancy query, cached)

    // Before a launch, on its stream: room for max_clusters workspaces, the block (allocated and zeroed whole on first use),
    // the control part zeroed.
    int prepare(hipStream_t stream, uint32_t max_clusters, size_t ws_per_cluster);
    ClusterCtl* ctl() const;
    ClusterStatus* status() const;
    // After a launch of `count` LWEs on e.stream: wait, read the status and, where the launch gave up, run the batch again on
    // the one-workgroup kernel.  With cfg.cluster_fallback off: leave it to the next check().
    int settle(Engine& e, const uint64_t* d_sm, const uint32_t* d_lut_idx, uint64_t* d_big, uint32_t count);
    int check();                      // after a synchronisation: did an unsettled launch give up on a hand-over?
    uint32_t last_clusters() const { return last; }   // fhe_engine_cluster_info
    uint32_t fallbacks() const { return n_fallbacks; }   // fhe_engine_cluster_fallbacks
};

// May a call take throughput mode 2 (whole calls overlapped on several streams) / mode 1 (its keyswitch in the shadow of the
// previous call's blind rotation)?  Asked by Engine::ks_pbs_dev.
bool overlapped_mode_eligible(const Engine& e, uint32_t count);
bool shadow_mode_eligible(const Engine& e, uint32_t count);

}  // namespace fhe
