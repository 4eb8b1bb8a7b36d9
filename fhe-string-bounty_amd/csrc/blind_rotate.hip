// blind_rotate.hip -- the blind-rotation kernels of libfhestr.so with everything that names one: the variant registry,
// the Fourier-key conversions, the dispatch (choose_rotate_path) and one launch function per path.  engine.hip holds the
// rest of the engine and reaches this file through engine.h and blind_rotate.h.
//
// Floating-point contraction: negacyclic_fft.hip.h, the first kernel header below, sets `#pragma clang fp contract(fast)` at
// file scope, so every kernel here and the host code of this file are compiled with fusion on (the command line says
// -ffp-contract=off; the pragma overrides it to the end of the translation unit).
#include "blind_rotate.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "engine.h"
#include "pbs_kernels.hip.h"
#include "pbs_dense_kernels.hip.h"
#include "pbs_large_kernels.hip.h"
#include "pbs_cluster_kernels.hip.h"
#include "pbs_xcd_kernels.hip.h"
#include "pbs_multibit_kernels.hip.h"
#include "pbs_seq_kernels.hip.h"

namespace fhe {

// ---- the variant registry: every descriptor is filled from its kernel's config struct ------------------------------------
constexpr int MASK_LDS_PER_N = 4;   // the modulus-switched mask in LDS: one u32 per small-LWE coefficient

template <class K>
static KernelRef kernel_ref(K* kernel, int threads, size_t lds_fixed, int lds_per_n = 0) {
    return {reinterpret_cast<const void*>(kernel), threads, lds_fixed, lds_per_n};
}

template <int LOGN, int LOGR, int K1, int L>
BrVariant make_variant() {
    using CFG = BrCfg<LOGN, LOGR, K1, L>;
    BrVariant v;
    v.logN = LOGN; v.k1 = K1; v.L = L; v.logR = LOGR; v.wide = false; v.large = false;
    v.rotate = kernel_ref(&blind_rotate_kernel<LOGN, LOGR, K1, L>, CFG::THREADS, CFG::LDS_FIXED, MASK_LDS_PER_N);
    v.convert = kernel_ref(&bsk_convert_kernel<LOGN, LOGR, K1, L>, CFG::THREADS, (size_t)K1 * CFG::GROUP_SLOTS * 8);
    return v;
}

template <int LOGN, int LOGR, int K1, int L>
BrVariant make_wide_variant() {
    using CFG = BrWideCfg<LOGN, LOGR, K1, L>;
    BrVariant v = make_variant<LOGN, LOGR, K1, L>();   // same Fourier key layout + conversion kernel
    v.wide = true;
    v.rotate = kernel_ref(&blind_rotate_wide_kernel<LOGN, LOGR, K1, L>, CFG::THREADS, CFG::LDS_FIXED, MASK_LDS_PER_N);
    if constexpr (CFG::OWN_PLAN) {        // FftSwap11 (N = 4096, where the wide variant is the shape's only one): the key in that plan's
                                          // order, one polynomial per workgroup
        v.convert = kernel_ref(&bsk_convert_wide_kernel<LOGN, LOGR, K1, L>, CFG::THREADS, (size_t)CFG::GROUP_SLOTS * 8);
        v.convert_one_per_block = true;
    }
    if constexpr (LOGN == 10 && LOGR == 2 && K1 == 3 && L == 1) {       // N = 1024, k = 2
        // single launches of 257 ... 512 LWEs: the wide kernel with the key prefetched, same launch shape
        v.rotate_keypf = kernel_ref(&blind_rotate_wide_kernel<LOGN, LOGR, K1, L, true>, CFG::THREADS, CFG::LDS_FIXED, MASK_LDS_PER_N);
        using DC = BrDenseCfg<LOGN, K1>;                                // pbs_dense_kernels.hip.h
        static_assert(DC::THREADS == CFG::THREADS, "same launch shape as the wide kernel");
        v.dense = kernel_ref(&blind_rotate_dense_kernel<LOGN, K1>, DC::THREADS, DC::LDS_FIXED, MASK_LDS_PER_N);
        v.dense_convert = kernel_ref(&bsk_convert_dense_kernel<LOGN, K1>, DC::THREADS, 0);
    }
    return v;
}

template <int LOGN, int K1, int L>
BrVariant make_large_variant() {
    using CFG = BrLargeCfg<LOGN, K1, L>;
    BrVariant v;
    v.logN = LOGN; v.k1 = K1; v.L = L; v.logR = 3; v.wide = false; v.large = true;
    v.rotate = kernel_ref(&blind_rotate_large_kernel<LOGN, K1, L>, CFG::THREADS, CFG::LDS_BYTES);   // the mask stays in HBM
    v.ws_bytes = CFG::WS_BYTES;
    v.convert = kernel_ref(&bsk_convert_large_kernel<LOGN, K1, L>, CFG::THREADS, CFG::LDS_BYTES);
    v.convert_ws = (size_t)CFG::P * 16;
    if constexpr (K1 == 2) {
        using CC = BrClusterCfg<LOGN, K1, L>;
        static_assert(CC::THREADS == CFG::THREADS, "same block size as the one-workgroup kernel");
        v.cluster = kernel_ref(&blind_rotate_cluster_kernel<LOGN, K1, L>, CC::THREADS, CC::LDS_BYTES, MASK_LDS_PER_N);
        v.cluster_size = CC::C;
        v.cluster_ws = CC::WS_BYTES;
        if constexpr (L == 2 && LOGN == 15) {
            using XC = BrXcdCfg<LOGN, K1, L>;
            v.xcd = kernel_ref(&blind_rotate_xcd_kernel<LOGN, K1, L>, XC::THREADS, XC::LDS_BYTES, MASK_LDS_PER_N);
            v.xcd_size = XC::C;
            v.xcd_ws = XC::WS_BYTES;
            v.xcd_lds_one_per_cu = XC::LDS_TWO_PER_CU + 1024;     // more than half of a CU's LDS: one workgroup per CU
        }
    }
    return v;
}

// N = 8192: transforms in LDS one polynomial at a time, accumulator in a cache-resident workspace (pbs_seq_kernels.hip.h)
template <int LOGN, int K1, int L>
BrVariant make_seq_variant() {
    using CFG = BrSeqCfg<LOGN, K1, L>;
    BrVariant v;
    v.logN = LOGN; v.k1 = K1; v.L = L; v.logR = 3; v.wide = false; v.large = true;
    v.rotate = kernel_ref(&blind_rotate_seq_kernel<LOGN, K1, L>, CFG::THREADS, CFG::LDS_FIXED, MASK_LDS_PER_N);
    v.ws_bytes = CFG::WS_BYTES;
    v.convert = kernel_ref(&bsk_convert_seq_kernel<LOGN, K1, L>, CFG::THREADS, CFG::LDS_CONVERT);
    v.convert_ws = 16;
    return v;
}

template <int LOGN, int LOGR, int K1, int G>
BrVariant make_multibit_variant() {
    using CFG = BrMultiBitCfg<LOGN, LOGR, K1, G>;
    BrVariant v = make_variant<LOGN, LOGR, K1, 1>();   // same Fourier key slot order + conversion kernel
    v.grouping = G;
    constexpr int DEGREES_LDS_PER_N = 4 * CFG::SEL / G + 4;         // (n/G) * (2^G - 1) degrees, rounded up
    v.rotate = kernel_ref(&blind_rotate_multibit_kernel<LOGN, LOGR, K1, G>, CFG::THREADS, CFG::LDS_FIXED, DEGREES_LDS_PER_N);
    v.rotate_combined = kernel_ref(&blind_rotate_multibit_kernel<LOGN, LOGR, K1, G, true>, CFG::THREADS, CFG::LDS_FIXED, DEGREES_LDS_PER_N);
    v.combine = kernel_ref(&multibit_combine_kernel<LOGN, LOGR, K1, G>, CFG::THREADS, CFG::LDS_ROOTS);
    v.combine_grid_y = CFG::R / CFG::COMBINE_SLOTS;
    v.combine_chunk = CFG::COMBINE_CHUNK;
    v.combined_bytes = (size_t)K1 * K1 * CFG::P * 16;
    return v;
}

// Multi-bit PBS for a shape served by the classic split / N = 8192 / large-N kernel (`v` from make_variant, make_seq_variant or make_large_variant):
// same Fourier key layout and conversion, rotation = that kernel's EXTPROD mode (same launch shape) against GGSWs prepared by
// multibit_combine_generic_kernel.
template <auto EXTPROD_KERNEL>
BrVariant make_multibit_two_kernel_variant(BrVariant v, int G) {
    using GC = MultiBitCombineGenericCfg;
    v.grouping = G;
    v.rotate.fn = reinterpret_cast<const void*>(EXTPROD_KERNEL);
    v.rotate_is_extprod = true;
    v.combine_generic = G == 2 ? kernel_ref(&multibit_combine_generic_kernel<2>, GC::THREADS, GC::lds_bytes((uint32_t)v.logN))
                               : kernel_ref(&multibit_combine_generic_kernel<3>, GC::THREADS, GC::lds_bytes((uint32_t)v.logN));
    v.combine_generic_elems = GC::ELEMS_PER_WG;
    v.combine_generic_chunk = GC::CHUNK;
    v.combined_bytes = (size_t)v.L * v.k1 * v.k1 * ((size_t)1 << (v.logN - 1)) * 16;
    return v;
}
template <int LOGN, int LOGR, int K1, int L>
BrVariant make_multibit_generic_variant(int G) {
    return make_multibit_two_kernel_variant<&blind_rotate_kernel<LOGN, LOGR, K1, L, true>>(make_variant<LOGN, LOGR, K1, L>(), G);
}
template <int LOGN, int K1, int L>
BrVariant make_multibit_seq_variant(int G) {
    return make_multibit_two_kernel_variant<&blind_rotate_seq_kernel<LOGN, K1, L, true>>(make_seq_variant<LOGN, K1, L>(), G);
}

static const std::vector<BrVariant>& variants() {
    static const std::vector<BrVariant> v = {
        // PARAM_MESSAGE_2_CARRY_2_KS_PBS: N=2048, k=1, l=1  (first entry of a shape = default)
        make_variant<11, 2, 2, 1>(), make_variant<11, 3, 2, 1>(), make_variant<11, 4, 2, 1>(),
        make_wide_variant<11, 2, 2, 1>(), make_wide_variant<11, 3, 2, 1>(),
        // PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS: multi-bit PBS, grouping factor 2
        make_multibit_variant<11, 2, 2, 2>(),
        // PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS: grouping factor 3 (8 GGSWs per group)
        make_multibit_variant<11, 2, 2, 3>(),
        // PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_{2,3}_KS_PBS (N = 512, k = 3) and
        // PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_{2,3}_KS_PBS (N = 8192, two levels): two-kernel path
        make_multibit_generic_variant<9, 2, 4, 1>(2), make_multibit_generic_variant<9, 2, 4, 1>(3),
        make_multibit_seq_variant<13, 2, 2>(2), make_multibit_seq_variant<13, 2, 2>(3),
        // toy shapes of the multi-bit tests (N = 256, k = 1, two levels; N = 128, k = 2)
        make_multibit_generic_variant<8, 2, 2, 2>(2), make_multibit_generic_variant<8, 2, 2, 2>(3),
        make_multibit_generic_variant<7, 2, 3, 1>(2), make_multibit_generic_variant<7, 2, 3, 1>(3),
        // N=1024, k=2, l=1 family (PARAM_MESSAGE_2_CARRY_1_KS_PBS ...)
        // (4 points per thread, 384 threads: 2.77 ms per 256 LWEs; 8 per thread, 192 threads: 3.38 ms)
        make_variant<10, 2, 3, 1>(), make_variant<10, 3, 3, 1>(), make_wide_variant<10, 2, 3, 1>(),
        // PARAM_MESSAGE_1_CARRY_1_KS_PBS: N=512, k=3, l=1
        make_variant<9, 2, 4, 1>(),
        // toy shapes used by the fast tests
        make_variant<8, 2, 2, 2>(), make_variant<7, 2, 3, 1>(),
        make_wide_variant<8, 2, 2, 2>(), make_wide_variant<7, 2, 3, 1>(),
        // the remaining *_KS_PBS shapes of shortint/parameters/mod.rs
        make_variant<8, 2, 6, 1>(),                                  // N = 256, k = 5  (1_CARRY_0)
        make_variant<9, 2, 3, 2>(),                                  // N = 512, k = 2, 2 levels (2_CARRY_0)
        make_wide_variant<12, 2, 2, 1>(), make_wide_variant<12, 2, 2, 2>(),   // N = 4096 (2_CARRY_3 ..., 1_CARRY_4)
        // polynomial sizes beyond the LDS: four-step FFT through an HBM workspace
        make_seq_variant<13, 2, 1>(), make_seq_variant<13, 2, 2>(),           // N = 8192  (5_CARRY_1 ..., 3_CARRY_3 ...)
        make_large_variant<14, 2, 2>(),                                       // N = 16384 (3_CARRY_4 ...)
        make_large_variant<15, 2, 2>(),                                       // N = 32768 (4_CARRY_4 ...)
        make_large_variant<14, 2, 3>(), make_large_variant<15, 2, 3>(),       // 3 levels of base 2^11 (1_CARRY_6, 3_CARRY_5 ...)
    };
    return v;
}

const BrVariant* find_variant(const fhe_params_t& p, int selector) {
    int logN = 0;
    while ((1u << logN) < p.N) logN++;
    const int logR = selector & 15;
    const bool wide = (selector & 16) != 0;
    const int grouping = p.grouping_factor > 1 ? (int)p.grouping_factor : 1;
    for (const auto& v : variants())
        if (v.logN == logN && v.k1 == (int)p.k + 1 && v.L == (int)p.pbs_level && v.grouping == grouping &&
            (selector == 0 || (v.logR == logR && v.wide == wide)))
            return &v;
    return nullptr;
}

BrVariantPair find_variant_pair(const fhe_params_t& p, int selector) {
    const BrVariant* v = find_variant(p, selector);
    const BrVariant* w = v && selector == 0 ? find_variant(p, v->logR | 16) : nullptr;
    return {v, w ? w : v};
}

// ---- Engine members that name a variant's kernel ------------------------------------------------------------------------
int Engine::set_variant(int logR) {
    const BrVariantPair vp = find_variant_pair(p, logR);
    if (!vp.small) return fail("no such blind-rotation variant for these parameters");
    if (d_fbsk && vp.small->logR != variant->logR)
        return fail("variant must be chosen before fhe_engine_load_keys (Fourier key layout depends on it)");
    variant = vp.small;
    variant_large = vp.large;
    shadow_fit = -1;
    return d_fbsk ? allow_rotate_lds() : 0;
}

int Engine::allow_rotate_lds() {
    for (const KernelRef* k : {&variant->rotate, &variant_large->rotate, &variant->rotate_combined})
        if (*k) HIP_TRY(hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k->lds(p.n)));
    return 0;
}

// Standard-domain polynomials -> the variant's Fourier layout (bsk_convert_kernel / bsk_convert_large_kernel).
int Engine::convert_polys(const uint64_t* d_std, double* d_out, uint32_t n_polys) {
    const uint32_t k1 = p.k + 1;
    const KernelRef& k = variant->convert;
    HIP_TRY(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds(p.n)));
    if (variant->large) {
        const uint32_t blocks = n_polys < (uint32_t)cu_count ? n_polys : (uint32_t)cu_count;
        DeviceBuffer<void> cws;
        if (cws.alloc((size_t)blocks * variant->convert_ws)) return 1;
        void* d_cws = cws;
        void* args[] = {(void*)&d_std, (void*)&d_out, (void*)&n_polys, (void*)&d_cws};
        if (under("bsk conversion", launch(k, dim3(blocks), args, p.n, stream))) return 1;
        return under("bsk conversion", hipStreamSynchronize(stream));
    }
    void* args[] = {(void*)&d_std, (void*)&d_out, (void*)&n_polys};
    HIP_TRY(launch(k, dim3(variant->convert_one_per_block ? n_polys : (n_polys + k1 - 1) / k1), args, p.n, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

// Which power of w = e^{i pi / N} each slot of the Fourier layout evaluates at: transform the monomial X with the
// variant's own conversion kernel and read the angles off (pbs_multibit_kernels.hip.h, "any other shape").
int Engine::probe_slot_exponents() {
    const uint32_t k1 = p.k + 1, P = p.N / 2;
    std::vector<uint64_t> mono((size_t)k1 * p.N, 0);
    for (uint32_t r = 0; r < k1; r++) mono[(size_t)r * p.N + 1] = 1;
    std::vector<double> spec((size_t)P * 2);
    {
        DeviceBuffer<uint64_t> d_mono;
        DeviceBuffer<double> d_spec;
        if (d_mono.alloc(mono.size() * 8) || d_spec.alloc(mono.size() * 8)) return 1;
        HIP_TRY(hipMemcpy(d_mono, mono.data(), mono.size() * 8, hipMemcpyHostToDevice));
        if (convert_polys(d_mono, d_spec, k1)) return 1;
        if (hipMemcpy(spec.data(), d_spec, spec.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("slot probe: copy");
    }
    std::vector<uint32_t> expo(P);
    const double pi = 3.14159265358979323846;
    for (uint32_t s = 0; s < P; s++) {
        const double turns = std::atan2(spec[2 * s + 1], spec[2 * s]) / pi * (double)p.N;   // in units of pi / N
        const long e = std::lround(turns);
        expo[s] = (uint32_t)(((e % (long)(2 * p.N)) + 2 * p.N) % (2 * p.N));
        if (std::fabs(turns - (double)e) > 0.01 || (expo[s] & 1) == 0)     // roots of X^N + 1 are the odd powers of w
            return fail("slot probe: the conversion kernel did not return a root of X^N + 1");
    }
    if (d_slot_exp.alloc((size_t)P * 4)) return 1;
    HIP_TRY(hipMemcpy(d_slot_exp, expo.data(), (size_t)P * 4, hipMemcpyHostToDevice));
    return 0;
}

// The copy of the key in the dense kernel's own Fourier order (FftSwap9; N = 1024, k = 2: 54.7 MB), where variant_large has that kernel.
int Engine::convert_dense_key(const uint64_t* d_std, uint32_t n_polys) {
    d_fbsk_dense.release();
    if (!variant_large->dense_convert) return 0;
    if (d_fbsk_dense.alloc((size_t)n_polys * p.N * 8)) return 1;
    void* cargs[] = {(void*)&d_std, (void*)&d_fbsk_dense.ptr, (void*)&n_polys};
    HIP_TRY(launch(variant_large->dense_convert, dim3(n_polys), cargs, p.n, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

// ---- blind-rotation dispatch: choose_rotate_path is the map, then one launch function per path ----------------------
enum class BrPath { Overlapped, MultiBitCombined, MultiBitTwoKernel, WholeXcd, Cluster, Large, Dense, Plain };

// Which path serves a batch, and (`v`) on which of the engine's two variants.  Reads cu_count and the dispatch settings
// of e.cfg (cluster_mode, cluster_max_batch, xcd_auto_max, multibit_combine_max, dense_per_cu) and whether d_fbsk_dense exists; calls
// no HIP function.  The order of the tests matters.  one_workgroup_only: the re-run of MultiCuRuntime::settle, never a multi-CU kernel.
static BrPath choose_rotate_path(const Engine& e, uint32_t count, bool two_per_cu, bool one_workgroup_only, const BrVariant*& v) {
    const EngineSettings& cfg = e.cfg;
    const uint32_t cus = (uint32_t)e.cu_count;
    // one LWE per CU or fewer: spread it over more threads; above that: the compact layout that lets two LWEs share a CU
    v = two_per_cu || count > cus ? e.variant_large : e.variant;
    if (two_per_cu) return BrPath::Overlapped;      // overlapped throughput mode: the compact layout whatever the batch size, on the given stream
    // far fewer LWEs than CUs: the idle CUs prepare the groups' GGSWs (lwe_multi_bit_programmable_bootstrapping.rs
    // splits the same way over CPU threads), the rotation then runs n/G plain external products
    if (v->combine && count <= cfg.multibit_combine_max) return BrPath::MultiBitCombined;
    // multi-bit PBS on a shape without a fused kernel: prepare the (LWE, group) GGSWs, then n/G external products per LWE
    if (v->rotate_is_extprod) return BrPath::MultiBitTwoKernel;
    // automatic mode: the whole-XCD kernel up to two LWEs per XCD (one LWE 12.3 ms, 16 LWEs 18.4 ms; the 8-CU clusters: 20.9 /
    // 21.4 ms), the 8-CU clusters above (256 LWEs: 1.15 k PBS/s against 0.85 k -- four LWEs in flight per XCD amortise the
    // hand-over latency better than two; profiles/r04_xcd_history.txt).  Mode 2: clusters, never the whole-XCD kernel.
    // (a device with fewer than 8 * C compute units -- e.g. one XCD of a partitioned GPU -- cannot host a grid of either
    // kernel: it takes the one-workgroup kernel below)
    const int mode = one_workgroup_only ? 0 : cfg.cluster_mode;
    if (v->xcd && mode != 0 && mode != 2 && (mode == 1 || count <= std::min(cfg.cluster_max_batch, cfg.xcd_auto_max)) &&
        cus >= 8u * (uint32_t)v->xcd_size)
        return BrPath::WholeXcd;
    if (v->cluster && mode != 0 && (mode >= 1 || count <= cfg.cluster_max_batch) && cus >= 8u * (uint32_t)v->cluster_size)
        return BrPath::Cluster;
    if (v->large) return BrPath::Large;      // polynomial beyond the LDS: one workgroup per LWE with an HBM workspace
    // more than two LWEs per CU: the variant that puts four on one
    if (v->dense && e.d_fbsk_dense && cfg.dense_per_cu && count > cfg.dense_per_cu * cus) return BrPath::Dense;
    return BrPath::Plain;
}

// May a call take throughput mode 2 (whole calls overlapped on several streams)?  Own stream only (a caller's stream is ordered by the caller); the
// rotation is the two-LWEs-per-CU twin of the primary variant, not multi-bit, at most one LWE per CU: two such launches then share every CU.
bool overlapped_mode_eligible(const Engine& e, uint32_t count) {
    return e.stream == e.own_stream && e.variant_large != e.variant && e.variant_large->wide && !e.variant->rotate_is_extprod &&
           !e.variant->combine && count <= (uint32_t)e.cu_count;
}
// May a call take throughput mode 1 (its keyswitch in the shadow of the previous call's blind rotation)?  Own stream only; the rotation is the plain
// launch of a variant neither wide nor large nor two-kernel multi-bit, at most one LWE per CU.  Engine::shadow_keyswitch_fits is asked as well.
bool shadow_mode_eligible(const Engine& e, uint32_t count) {
    return e.stream == e.own_stream && !e.variant->large && !e.variant->wide && !e.variant->rotate_is_extprod && count <= (uint32_t)e.cu_count;
}

static int rotate_overlapped(Engine& e, const BrVariant* w, BlindRotateArgs a, hipStream_t on) {
    a.fair_shift = e.cfg.wide_fair_shift;      // the two launches that share the GPU progress at the same rate (110 k -> 122 k PBS/s)
    void* args[] = {(void*)&a};
    HIP_TRY(launch(w->rotate, dim3(a.batch), args, e.p.n, on));
    return 0;
}

static int rotate_multibit_combined(Engine& e, const BrVariant* v, const BlindRotateArgs& a) {
    const size_t groups = e.p.n / e.p.grouping_factor;
    if (e.d_ws.reserve((size_t)a.batch * groups * v->combined_bytes)) return 1;
    MultiBitCombineArgs ca{a, reinterpret_cast<double2*>(e.d_ws.ptr)};
    if (e.one_span("multi-bit combine", (a.batch + v->combine_chunk - 1) / v->combine_chunk, 2)) return 1;   // grid.z = chunks of the batch: at most multibit_combine_max LWEs take this path
    void* cargs[] = {(void*)&ca};
    HIP_TRY(launch(v->combine, dim3((unsigned)groups, (unsigned)v->combine_grid_y, (a.batch + v->combine_chunk - 1) / v->combine_chunk), cargs,
                   e.p.n, e.stream));
    BlindRotateArgs b = a;
    b.fbsk = reinterpret_cast<const double*>(e.d_ws.ptr);
    void* bargs[] = {(void*)&b};
    HIP_TRY(launch(v->rotate_combined, dim3(a.batch), bargs, e.p.n, e.stream));
    return 0;
}

// Sub-batches keep the prepared GGSWs within a fixed workspace.
static int rotate_multibit_two_kernel(Engine& e, const BrVariant* v, const BlindRotateArgs& a) {
    const fhe_params_t& p = e.p;
    const uint32_t count = a.batch;
    const size_t groups = p.n / p.grouping_factor, per_lwe = groups * v->combined_bytes;
    const size_t rot_ws = v->large ? v->ws_bytes : 0;
    size_t cap = e.cfg.multibit_workspace_cap;
    if (cap == 0) {       // automatic: half of what is free now (plus what the workspace already holds), at most 64 GB
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        cap = std::min<size_t>((size_t)64 << 30, (free_b + e.d_ws.bytes) / 2);
    }
    const uint32_t sub_max = (uint32_t)std::max<size_t>(1, std::min<size_t>(count, cap / (per_lwe + rot_ws)));
    if (e.d_ws.reserve((size_t)sub_max * (per_lwe + rot_ws))) return 1;
    unsigned char* rot_base = e.d_ws + (size_t)sub_max * per_lwe;
    const uint32_t logN = (uint32_t)v->logN, ggsw_elems = (uint32_t)(v->combined_bytes / 16);
    const uint32_t per_wg = (uint32_t)v->combine_generic_elems, chunk = (uint32_t)v->combine_generic_chunk;
    const size_t big = (size_t)p.k * p.N + 1;
    for (uint32_t first = 0; first < count; first += sub_max) {
        const uint32_t sub = std::min(sub_max, count - first);
        MultiBitCombineGenericArgs ca{a.lwe_small + (size_t)first * (p.n + 1), reinterpret_cast<const double2*>(e.d_fbsk.ptr), e.d_slot_exp,
                                      reinterpret_cast<double2*>(e.d_ws.ptr), p.n, logN, p.N / 2, ggsw_elems, sub};
        void* cargs[] = {(void*)&ca};
        if (e.one_span("multi-bit combine", (ggsw_elems + per_wg - 1) / per_wg, 1) || e.one_span("multi-bit combine", (sub + chunk - 1) / chunk, 2)) return 1;
        HIP_TRY(launch(v->combine_generic, dim3((unsigned)groups, (ggsw_elems + per_wg - 1) / per_wg, (sub + chunk - 1) / chunk), cargs, p.n, e.stream));
        BlindRotateLargeArgs la{{a.lwe_small + (size_t)first * (p.n + 1), a.lut_idx ? a.lut_idx + first : nullptr, a.luts,
                                 reinterpret_cast<const double*>(e.d_ws.ptr), a.lwe_out + (size_t)first * big, p.n, p.pbs_base_log, sub,
                                 p.grouping_factor}, rot_base};
        void* largs[] = {v->large ? (void*)&la : (void*)&la.base};      // the HBM-workspace kernels take theirs behind the same arguments
        HIP_TRY(launch(v->rotate, dim3(sub), largs, p.n, e.stream));
    }
    return 0;
}

// Several CUs per LWE (the whole-XCD kernel and the 8-CU clusters): the grid is a whole number of 8 * C workgroups (the
// dispatcher deals workgroups round-robin over the 8 XCDs, the kernel forms its clusters from what each XCD actually
// received) and every workgroup of it must be resident at once: `rounds` workgroups per CU, no more.
static int rotate_multi_cu(Engine& e, const BlindRotateArgs& a, const KernelRef& k, uint32_t C, size_t lds_one_per_cu, size_t ws_per_cluster,
                           uint32_t rounds) {
    const uint32_t quantum = 8 * C;
    const uint32_t max_clusters = std::min<uint32_t>((uint32_t)CLUSTER_MAX, ((uint32_t)e.cu_count / quantum) * 8 * rounds);
    const uint32_t grid = (std::min(a.batch, max_clusters) + 7) / 8 * quantum;
    const size_t lds = grid <= (uint32_t)e.cu_count ? std::max(k.lds(e.p.n), lds_one_per_cu) : k.lds(e.p.n);
    MultiCuRuntime& rt = e.multi_cu;
    if (rt.prepare(e.stream, max_clusters, ws_per_cluster)) return 1;
    BlindRotateClusterArgs ka{a, rt.ws, rt.ctl(), rt.status(), e.cfg.cluster_spin_limit, e.cfg.cluster_test_fault};
    void* kargs[] = {(void*)&ka};
    HIP_TRY(launch(k, dim3(grid), kargs, e.p.n, e.stream, lds));
    return rt.settle(e, a.lwe_small, a.lut_idx, a.lwe_out, a.batch);
}

// All CUs of an XCD per LWE (pbs_xcd_kernels.hip.h).  Up to 8 LWEs: one cluster per XCD, one 256-thread workgroup
// per CU (the dynamic LDS request is padded past half a CU's LDS so that no CU takes two).  More: two clusters per
// XCD, i.e. two workgroups on every CU -- the grid is exactly what the device holds.
static int rotate_whole_xcd(Engine& e, const BrVariant* v, const BlindRotateArgs& a) {
    int& xcd_per_cu = e.multi_cu.xcd_per_cu;
    if (xcd_per_cu < 0) {       // once per engine: do two of its workgroups fit a CU?  (registers, LDS: asked, not assumed)
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, v->xcd.fn, v->xcd.threads, v->xcd.lds(e.p.n)));
        xcd_per_cu = per_cu;
    }
    const uint32_t rounds = (a.batch > 8 && xcd_per_cu >= 2) ? 2u : 1u;
    return rotate_multi_cu(e, a, v->xcd, (uint32_t)v->xcd_size, v->xcd_lds_one_per_cu, v->xcd_ws, rounds);
}

static int rotate_large(Engine& e, const BrVariant* v, const BlindRotateArgs& a) {
    if (e.d_ws.reserve((size_t)a.batch * v->ws_bytes)) return 1;
    BlindRotateLargeArgs la{a, e.d_ws};
    void* largs[] = {(void*)&la};
    HIP_TRY(launch(v->rotate, dim3(a.batch), largs, e.p.n, e.stream));
    return 0;
}

static int rotate_dense(Engine& e, const BrVariant* v, BlindRotateArgs a) {
    a.fair_shift = 0;
    a.fbsk = e.d_fbsk_dense;
    void* args[] = {(void*)&a};
    HIP_TRY(launch(v->dense, dim3(a.batch), args, e.p.n, e.stream));
    return 0;
}

static int rotate_plain(Engine& e, const BrVariant* v, BlindRotateArgs a) {
    uint32_t grid = a.batch;
    // keep-busy mode (fhe_engine_set_keep_busy): a launch that would leave more than half of the CUs idle carries replicas of
    // its workgroups on them (they recompute and store nothing) -- the part then keeps its clock for the large launch that
    // follows (2.22 -> 2.39 GHz over 14 ms otherwise, profiles/r03_after_idle.txt), at the price of the energy
    if (e.cfg.keep_busy && !v->wide && !v->large && a.batch * 2 <= (uint32_t)e.cu_count) grid = a.batch * ((uint32_t)e.cu_count / a.batch);
    void* args[] = {(void*)&a};
    HIP_TRY(launch(v->rotate_keypf && v->wide ? v->rotate_keypf : v->rotate, dim3(grid), args, e.p.n, e.stream));
    return 0;
}

int Engine::launch_blind_rotate(const uint64_t* d_sm, const uint32_t* d_lut_idx, uint64_t* d_big, uint32_t count, hipStream_t on,
                                bool two_per_cu, bool one_workgroup_only) {
    if (!d_fbsk) return fail("keys not loaded");
    if (n_luts == 0) return fail("no lookup table uploaded");
    BlindRotateArgs a{d_sm, d_lut_idx, d_luts, d_fbsk, d_big, p.n, p.pbs_base_log, count};
    a.grouping = 0;
    // two-LWEs-per-CU kernel: fair time-sliced priorities when every CU gets an even number of workgroups (pbs_kernels.hip.h)
    const uint32_t cus = (uint32_t)cu_count;
    a.fair_shift = (count > cus && (((count + cus - 1) / cus) & 1u) == 0) ? cfg.wide_fair_shift : 0u;
    const BrVariant* v = nullptr;
    switch (choose_rotate_path(*this, count, two_per_cu, one_workgroup_only, v)) {
        case BrPath::Overlapped: return rotate_overlapped(*this, v, a, on ? on : stream);
        case BrPath::MultiBitCombined: return rotate_multibit_combined(*this, v, a);
        case BrPath::MultiBitTwoKernel: return rotate_multibit_two_kernel(*this, v, a);
        case BrPath::WholeXcd: return rotate_whole_xcd(*this, v, a);
        case BrPath::Cluster:       // 8-CU clusters (pbs_cluster_kernels.hip.h): never more than one workgroup per CU
            return rotate_multi_cu(*this, a, v->cluster, (uint32_t)v->cluster_size, 0, v->cluster_ws, 1);
        case BrPath::Large: return rotate_large(*this, v, a);
        case BrPath::Dense: return rotate_dense(*this, v, a);
        case BrPath::Plain: break;
    }
    return rotate_plain(*this, v, a);
}

// Can a 64-register keyswitch wave sit on a SIMD next to the blind rotation's waves?  (one workgroup per CU, its waves
// spread over the four SIMDs, registers allocated in blocks of 8 out of 512 per SIMD lane)
bool Engine::shadow_keyswitch_fits() {
    if (shadow_fit < 0) {
        hipFuncAttributes fa{};
        shadow_fit = 0;
        if (hipFuncGetAttributes(&fa, variant->rotate.fn) == hipSuccess) {
            const int waves_per_simd = (variant->rotate.threads / 64 + 3) / 4;
            const int regs = (fa.numRegs + 7) / 8 * 8;
            shadow_fit = waves_per_simd * regs + 64 <= 512 ? 1 : 0;
        }
    }
    return shadow_fit == 1;
}

uint32_t Engine::rotate_registers() const {
    hipFuncAttributes fa{};
    return variant && hipFuncGetAttributes(&fa, variant->rotate.fn) == hipSuccess ? (uint32_t)fa.numRegs : 0u;
}

// ---- MultiCuRuntime ---------------------------------------------------------------------------------------------------
int MultiCuRuntime::prepare(hipStream_t stream, uint32_t max_clusters, size_t ws_per_cluster) {
    if (ws.reserve((size_t)max_clusters * ws_per_cluster)) return 1;
    if (!block) {
        if (block.alloc(sizeof(ClusterCtl) + sizeof(ClusterStatus))) return 1;
        HIP_TRY(hipMemsetAsync(block, 0, sizeof(ClusterCtl) + sizeof(ClusterStatus), stream));
    }
    // tickets and flags start from zero; the status words behind them are sticky (read by settle() / check())
    HIP_TRY(hipMemsetAsync(block, 0, sizeof(ClusterCtl), stream));
    return 0;
}

ClusterCtl* MultiCuRuntime::ctl() const { return static_cast<ClusterCtl*>(block.ptr); }
ClusterStatus* MultiCuRuntime::status() const { return reinterpret_cast<ClusterStatus*>(ctl() + 1); }

// The cluster kernel never hangs on a hand-over that does not arrive: it gives up, finishes with garbage and says so
// in its status words.  Every host-visible completion point asks here.
// A launch of one of the multi-CU kernels is settled before the call returns: the host waits for it, reads the
// status words and, when the formation or a hand-over gave up -- a foreign kernel held compute units the grid needed;
// the kernel drained with invalid results instead of hanging -- runs the same batch on the one-workgroup kernel, which
// needs nothing resident but itself.  These kernels take 10 ms and more per launch: the synchronisation costs nothing
// measurable.  FHESTR_CLUSTER_FALLBACK=0: the round-3 behaviour (checked at the next completion point, reported as an error).
int MultiCuRuntime::settle(Engine& e, const uint64_t* d_sm, const uint32_t* d_lut_idx, uint64_t* d_big, uint32_t count) {
    if (!e.cfg.cluster_fallback) { unchecked = true; return 0; }
    ClusterStatus st{};
    HIP_TRY(hipMemcpyAsync(&st, status(), sizeof(st), hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    last = st.clusters;
    if (!st.error) return 0;
    HIP_TRY(hipMemsetAsync(status(), 0, sizeof(st), e.stream));
    n_fallbacks++;
    last_error = st.error;
    return e.launch_blind_rotate(d_sm, d_lut_idx, d_big, count, nullptr, false, /*one_workgroup_only=*/true);
}

int MultiCuRuntime::check() {
    if (!unchecked || !block) return 0;
    ClusterStatus st{};
    HIP_TRY(hipMemcpy(&st, status(), sizeof(st), hipMemcpyDeviceToHost));
    unchecked = false;
    last = st.clusters;
    if (st.error) {
        HIP_TRY(hipMemset(status(), 0, sizeof(st)));
        return fail("blind_rotate_cluster_kernel: a cluster hand-over timed out (code " + std::to_string(st.error) +
                    "); results of that launch are invalid");
    }
    return 0;
}

#ifdef FHESTR_WALL
extern "C" int fhe_debug_read_wall(unsigned long long* out, size_t count) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wall), count * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif
#ifdef FHESTR_STAMPS
extern "C" int fhe_debug_read_stamps(unsigned long long* out, size_t count) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), count * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif

}  // namespace fhe
