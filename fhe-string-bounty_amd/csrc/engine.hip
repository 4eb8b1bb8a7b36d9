// engine.hip -- host side of libfhestr.so: device memory, key residency, the keyswitch launches (with the matrix-core launch
// pieces the packing keyswitch shares: ks_mfma_launch.h) and the ks_pbs pipeline.  The blind-rotation kernels, their variant
// registry and their launches are blind_rotate.hip's; this file sees a variant's shape flags through blind_rotate.h.  The
// packed-ciphertext family (pack, unpack, narrow) is fhe::Packing's, in packing_dev.hip.
//
// The reference keeps a ServerKey {key_switching_key, bootstrapping_key (Fourier)} in host memory
// and runs one ciphertext at a time through thread-local scratch
// (shortint/server_key/mod.rs:783-857, shortint/engine/mod.rs:184-234).  Here the keys are made
// resident in HBM once (BSK 48.6 MB + KSK 60.9 MB for PARAM_MESSAGE_2_CARRY_2: both sit in the
// 256 MB Infinity Cache) and whole batches of LWEs go through three launches on one HIP stream:
// memset -> keyswitch (ks_decompose + keyswitch_mfma_kernel) -> blind rotation.
//
// Floating-point contraction: off for all device and host code of this file (-ffp-contract=off, and keygen_kernels.hip.h's own
// pragma for the bit-reproducible key generation of det_math.h); no header included here turns it on.
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "blind_rotate.h"
#include "keygen_kernels.hip.h"
#include "lwe_kernels.hip.h"
#include "ks_mfma_launch.h"
#include "ks_mfma_prep_kernels.hip.h"
#include "seeded_kernels.hip.h"
#include "compact_kernels.hip.h"

namespace fhe {

thread_local std::string g_last_error;

int fail(const std::string& msg) {
    g_last_error = msg;
    return 1;
}

// ---- Engine -----------------------------------------------------------------------------------
// Everything Engine::create checks before it touches a device: shapes the kernels are instantiated for, decomposition
// ranges of the keyswitch paths (any level count: more than 16 levels take the byte-plane kernel, ks_mfma_supported).
int params_supported(const fhe_params_t& p, int selector) {
    if ((p.N & (p.N - 1)) || p.N < 128) return fail("polynomial size must be a power of two >= 128");
    if (p.pbs_base_log < 1 || p.pbs_base_log > 31 || p.pbs_base_log * p.pbs_level > (p.pbs_level >= 3 ? 62u : 31u))
        return fail("unsupported PBS decomposition (base_log * level must be <= 31, or <= 62 with >= 3 levels)");
    if (p.ks_level < 1 || p.ks_base_log < 1 || p.ks_base_log > 7 || p.ks_base_log * p.ks_level > 62)
        return fail("unsupported keyswitch decomposition (base_log 1..7, base_log * level <= 62)");
    if (p.msg_mod * p.carry_mod == 0 || (p.N % (p.msg_mod * p.carry_mod)) != 0)
        return fail("msg_mod * carry_mod must divide N");
    if (p.grouping_factor > 1 && (p.n % p.grouping_factor) != 0) return fail("grouping factor must divide n");
    if (!find_variant(p, selector)) return fail("no blind-rotation kernel instantiated for this (N, k, level, grouping factor)");
    return 0;
}
int params_supported(const fhe_params_t& p) { return params_supported(p, 0); }

int Engine::create(const fhe_params_t& p, int device, Engine** out) {
    const EngineSettings cfg = EngineSettings::from_env();   // defaults, ranges and environment names: engine_settings.h
    if (params_supported(p, cfg.variant_selector)) return 1;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count <= 0) return fail("no HIP device: libfhestr has no CPU fallback");
    if (device < 0 || device >= count) return fail("bad device index");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<Engine> e(new Engine());   // freed by every early return below
    e->p = p;
    e->device = device;
    const BrVariantPair vp = find_variant_pair(p, cfg.variant_selector);
    e->variant = vp.small;
    e->variant_large = vp.large;
    e->cfg = cfg;
    e->pipe.width = cfg.overlap_width;
    e->packing.e = e.get();
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    e->cu_count = prop.multiProcessorCount;
    for (int q = 0; q < 3; q++) e->max_grid[q] = prop.maxGridSize[q] > 0 ? (uint32_t)prop.maxGridSize[q] : 0u;
    HIP_TRY(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    e->stream = e->own_stream;
    *out = e.release();
    return 0;
}

Engine::~Engine() {
    (void)hipSetDevice(device);
    if (stream) (void)sync_all_streams();
    transciphers.clear();
    cast_keys.clear();
    for (auto& e : ring) if (e) (void)hipEventDestroy(e);
    pipe.destroy();
    if (own_stream) (void)hipStreamDestroy(own_stream);
    // the members are destroyed after this body: every DeviceBuffer is freed once the streams are idle and gone
}

int Engine::set_stream(hipStream_t s, bool use_own) {
    if (use()) return 1;
    if (sync_all_streams()) return 1;
    stream = use_own ? own_stream : s;   // s == nullptr is HIP's default (null) stream
    return 0;
}

int Engine::lut_upload_dedup(const std::vector<uint64_t>& acc, uint32_t* id) {
    auto it = lut_dedup.find(acc);
    if (it != lut_dedup.end()) { *id = it->second; return 0; }
    if (lut_upload(acc.data(), id)) return 1;
    lut_dedup[acc] = *id;
    return 0;
}

int Engine::use() { HIP_TRY(hipSetDevice(device)); return 0; }

int Engine::load_keys(const uint64_t* bsk_std, const uint64_t* ksk) {
    if (use()) return 1;
    const size_t ksk_len = (size_t)p.k * p.N * p.ks_level * (p.n + 1);
    const size_t bsk_len = (size_t)n_ggsw(p) * p.pbs_level * (p.k + 1) * (p.k + 1) * p.N;
    DeviceBuffer<uint64_t> d_ksk_std, d_bsk_std;
    if (d_ksk_std.alloc(ksk_len * 8) || d_bsk_std.alloc(bsk_len * 8)) return 1;
    if (under("key upload", hipMemcpyAsync(d_ksk_std, ksk, ksk_len * 8, hipMemcpyHostToDevice, stream)) ||
        under("key upload", hipMemcpyAsync(d_bsk_std, bsk_std, bsk_len * 8, hipMemcpyHostToDevice, stream)))
        return 1;
    return install_keys(std::move(d_ksk_std), std::move(d_bsk_std));
}

// A tfhe-rs client's CompressedServerKey (shortint/server_key/compressed.rs): upload the bodies, expand the masks from
// the two compression seeds on the device (seeded_kernels.hip.h), then install as usual.
int Engine::load_seeded_keys(const uint8_t ksk_seed[16], const uint64_t* ksk_bodies, const uint8_t bsk_seed[16],
                             const uint64_t* bsk_bodies, uint64_t* bsk_std_out, uint64_t* ksk_out) {
    if (use()) return 1;
    const uint64_t ksk_rows = (uint64_t)p.k * p.N * p.ks_level, bsk_rows = (uint64_t)n_ggsw(p) * p.pbs_level * (p.k + 1);
    const size_t ksk_len = ksk_rows * (p.n + 1), bsk_len = bsk_rows * (p.k + 1) * p.N;
    const size_t bsk_body_words = bsk_rows * p.N;
    const char* const who = "load_seeded_keys";
    DeviceBuffer<uint64_t> d_ksk_std, d_bsk_std, d_bodies;
    DeviceBuffer<uint8_t> d_sbox;
    if (under(who, d_ksk_std.alloc(ksk_len * 8)) || under(who, d_bsk_std.alloc(bsk_len * 8)) ||
        under(who, d_bodies.alloc((bsk_body_words + ksk_rows) * 8)) || under(who, d_sbox.alloc(256)) ||
        under(who, hipMemcpyAsync(d_sbox, aes_sbox(), 256, hipMemcpyHostToDevice, stream)) ||
        under(who, hipMemcpyAsync(d_bodies, bsk_bodies, bsk_body_words * 8, hipMemcpyHostToDevice, stream)) ||
        under(who, hipMemcpyAsync(d_bodies + bsk_body_words, ksk_bodies, ksk_rows * 8, hipMemcpyHostToDevice, stream)))
        return 1;
    SeededExpandArgs ka{}, ba{};
    aes128_round_keys(ksk_seed, ka.round_keys);
    ka.out = d_ksk_std; ka.rows = ksk_rows; ka.mask_per_row = p.n; ka.row_words = p.n + 1;
    aes128_round_keys(bsk_seed, ba.round_keys);
    ba.out = d_bsk_std; ba.rows = bsk_rows; ba.mask_per_row = p.k * p.N; ba.row_words = (p.k + 1) * p.N;
    const unsigned grid = (unsigned)cu_count * 8;
    hipLaunchKernelGGL(seeded_expand_kernel, dim3(grid), dim3(256), 0, stream, ka, d_sbox.ptr);
    hipLaunchKernelGGL(seeded_expand_kernel, dim3(grid), dim3(256), 0, stream, ba, d_sbox.ptr);
    hipLaunchKernelGGL(seeded_scatter_bodies_kernel, dim3(grid), dim3(256), 0, stream, d_bodies + bsk_body_words, d_ksk_std.ptr, ksk_rows,
                       p.n, p.n + 1);
    hipLaunchKernelGGL(seeded_scatter_bodies_kernel, dim3(grid), dim3(256), 0, stream, d_bodies.ptr, d_bsk_std.ptr, bsk_rows, p.k * p.N,
                       (p.k + 1) * p.N);
    if (under(who, hipGetLastError()) ||
        (ksk_out && under(who, hipMemcpyAsync(ksk_out, d_ksk_std, ksk_len * 8, hipMemcpyDeviceToHost, stream))) ||
        (bsk_std_out && under(who, hipMemcpyAsync(bsk_std_out, d_bsk_std, bsk_len * 8, hipMemcpyDeviceToHost, stream))) ||
        under(who, hipStreamSynchronize(stream)))
        return 1;
    d_bodies.release();      // before install_keys allocates the Fourier key: key loading peaks no higher than it must
    d_sbox.release();
    return install_keys(std::move(d_ksk_std), std::move(d_bsk_std));
}

// Compressed big-key ciphertexts -> full ciphertexts in HBM (d_out, count x (kN+1) words) and/or host_out.
int Engine::expand_seeded_lwe(const uint8_t* seeds, const uint64_t* bodies, uint32_t count, uint64_t* d_out, uint64_t* host_out) {
    if (use()) return 1;
    if (count == 0) return 0;
    const uint32_t dim = p.k * p.N;
    const size_t words = (size_t)count * (dim + 1);
    const char* const who = "expand_seeded_lwe";
    DeviceBuffer<uint8_t> d_seeds, d_sbox;
    DeviceBuffer<uint64_t> d_bodies, d_tmp;
    if (under(who, d_seeds.alloc((size_t)count * 16)) || under(who, d_sbox.alloc(256)) || under(who, d_bodies.alloc((size_t)count * 8)) ||
        (!d_out && under(who, d_tmp.alloc(words * 8))) ||
        under(who, hipMemcpyAsync(d_seeds, seeds, (size_t)count * 16, hipMemcpyHostToDevice, stream)) ||
        under(who, hipMemcpyAsync(d_sbox, aes_sbox(), 256, hipMemcpyHostToDevice, stream)) ||
        under(who, hipMemcpyAsync(d_bodies, bodies, (size_t)count * 8, hipMemcpyHostToDevice, stream)))
        return 1;
    uint64_t* target = d_out ? d_out : d_tmp.ptr;
    hipLaunchKernelGGL(seeded_lwe_expand_kernel, dim3(count), dim3(64), 0, stream, d_seeds.ptr, d_bodies.ptr, d_sbox.ptr, target, dim);
    if (under(who, hipGetLastError()) || (host_out && under(who, hipMemcpyAsync(host_out, target, words * 8, hipMemcpyDeviceToHost, stream))))
        return 1;
    return under(who, hipStreamSynchronize(stream));
}

// A public-key client's compact ciphertext list (shortint CompactCiphertextList, compact_kernels.hip.h) -> count big-key
// ciphertexts at d_out.  d_list is ordered on the engine's stream like everything else; nothing synchronises.
int Engine::expand_compact_list_dev(const uint64_t* d_list, uint32_t count, uint64_t* d_out) {
    if (use()) return 1;
    if (count == 0) return 0;
    const uint32_t dim = p.k * p.N;
    if (dim < 2 || (dim & (dim - 1))) return fail("compact lists need a power-of-two encryption key dimension, k*N = " + std::to_string(dim));
    const uint32_t chunks = (dim / 2 + COMPACT_PAIRS_PER_WG - 1) / COMPACT_PAIRS_PER_WG;
    if ((uint64_t)count * chunks > 0x7FFFFFFFull) return fail("expand_compact_list: too many ciphertexts for one launch");
    hipLaunchKernelGGL(compact_expand_kernel, dim3(count * chunks), dim3(256), 0, stream, d_list, d_out, dim, count, chunks);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The same from a host list: 8 (ceil(count / kN) kN + count) bytes go over PCIe instead of 8 count (kN + 1).
// Output on the device (d_out) and / or the host; synchronises, like expand_seeded_lwe.
int Engine::expand_compact_list(const uint64_t* list, uint32_t count, uint64_t* d_out, uint64_t* host_out) {
    if (use()) return 1;
    if (count == 0) return 0;
    const uint32_t dim = p.k * p.N;
    if (dim < 2 || (dim & (dim - 1))) return fail("compact lists need a power-of-two encryption key dimension, k*N = " + std::to_string(dim));
    const size_t list_words = (size_t)((count + dim - 1) / dim) * dim + count, words = (size_t)count * (dim + 1);
    const char* const who = "expand_compact_list";
    if (d_compact.reserve(list_words * 8)) return 1;
    DeviceBuffer<uint64_t> d_tmp;
    if (!d_out && d_tmp.alloc(words * 8)) return 1;
    uint64_t* target = d_out ? d_out : d_tmp.ptr;
    if (under(who, hipMemcpyAsync(d_compact, list, list_words * 8, hipMemcpyHostToDevice, stream))) return 1;
    if (expand_compact_list_dev(d_compact, count, target)) return 1;
    if (host_out && under(who, hipMemcpyAsync(host_out, target, words * 8, hipMemcpyDeviceToHost, stream))) return 1;
    return under(who, hipStreamSynchronize(stream));
}

// Server-key generation on the device (keygen_kernels.hip.h); replaces ServerKey::new
// (shortint/engine/server_side.rs:54-160) for callers that hold the secret keys next to the GPU.
int Engine::generate_keys(const uint64_t* glwe_sk, const uint64_t* small_sk, const uint8_t seed[32],
                          uint64_t* bsk_std_out, uint64_t* ksk_out) {
    if (use()) return 1;
    const size_t in_dim = (size_t)p.k * p.N;
    const size_t ksk_len = in_dim * p.ks_level * (p.n + 1);
    const size_t bsk_len = (size_t)n_ggsw(p) * p.pbs_level * (p.k + 1) * (p.k + 1) * p.N;
    for (size_t i = 0; i < in_dim; i++)
        if (glwe_sk[i] > 1) return fail("glwe_sk must be binary");
    for (size_t i = 0; i < p.n; i++)
        if (small_sk[i] > 1) return fail("small_sk must be binary");
    // plaintext bit of every GGSW: the key bits themselves, or their per-group products (multi-bit)
    const uint32_t ng = n_ggsw(p), gf = p.grouping_factor > 1 ? p.grouping_factor : 1;
    std::vector<uint64_t> bits(ng);
    for (uint32_t i = 0; i < ng; i++)
        bits[i] = gf == 1 ? small_sk[i] : multi_bit_key_bit(small_sk + (size_t)(i >> gf) * gf, gf, i & ((1u << gf) - 1));
    const char* const who = "generate_keys";
    DeviceBuffer<uint64_t> d_gsk, d_ssk, d_bits, d_ksk_std, d_bsk_std;
    if (under(who, d_gsk.alloc(in_dim * 8)) || under(who, d_ssk.alloc((size_t)p.n * 8)) || under(who, d_bits.alloc((size_t)ng * 8)) ||
        under(who, hipMemcpyAsync(d_bits, bits.data(), (size_t)ng * 8, hipMemcpyHostToDevice, stream)) ||
        under(who, d_ksk_std.alloc(ksk_len * 8)) || under(who, d_bsk_std.alloc(bsk_len * 8)) ||
        under(who, hipMemcpyAsync(d_gsk, glwe_sk, in_dim * 8, hipMemcpyHostToDevice, stream)) ||
        under(who, hipMemcpyAsync(d_ssk, small_sk, (size_t)p.n * 8, hipMemcpyHostToDevice, stream)))
        return 1;
    KeygenArgs a{d_gsk, d_ssk, d_bits, d_ksk_std, d_bsk_std, seed_from_bytes(seed), p.n, p.k, p.N,
                 p.pbs_base_log, p.pbs_level, p.ks_base_log, p.ks_level, p.lwe_std, p.glwe_std};
    hipLaunchKernelGGL(ksk_gen_kernel, dim3((unsigned)((in_dim + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(bsk_gen_kernel, dim3(ng), dim3(256), 0, stream, a);
    if (under(who, hipGetLastError()) ||
        (ksk_out && under(who, hipMemcpyAsync(ksk_out, d_ksk_std, ksk_len * 8, hipMemcpyDeviceToHost, stream))) ||
        (bsk_std_out && under(who, hipMemcpyAsync(bsk_std_out, d_bsk_std, bsk_len * 8, hipMemcpyDeviceToHost, stream))) ||
        under(who, hipStreamSynchronize(stream)))
        return 1;
    d_gsk.release();      // as in load_seeded_keys: gone before install_keys allocates
    d_ssk.release();
    d_bits.release();
    return install_keys(std::move(d_ksk_std), std::move(d_bsk_std));
}

// Takes ownership of the two standard-domain device buffers: repacks the KSK into byte planes and
// converts the BSK to the active variant's Fourier layout; they are released when it returns, on every path.
int Engine::install_keys(DeviceBuffer<uint64_t>&& ksk_std, DeviceBuffer<uint64_t>&& bsk_std) {
    const DeviceBuffer<uint64_t> d_ksk_std = std::move(ksk_std), d_bsk_std = std::move(bsk_std);
    const uint64_t* d_std = d_bsk_std;
    const size_t bsk_len = (size_t)n_ggsw(p) * p.pbs_level * (p.k + 1) * (p.k + 1) * p.N;
    d_fbsk.release();
    {   // repack into byte planes once
        const uint32_t rows = p.k * p.N * p.ks_level, osz = p.n + 1;
        if (d_ksk_packed.alloc((size_t)(rows / 4) * 8 * osz * 4)) return 1;
        // grid.y = quads of key rows: k N ks_level / 4 reaches 90112 (PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_PBS_KS), so one launch
        // per span of the device's grid.y, each on its own rows of both arrays (the kernel sees a shorter key)
        const GridSpans quads = spans(rows / 4, 1);
        if (!quads.spans) return fail("install_keys: the device reports no grid.y");
        for (uint64_t i = 0; i < quads.spans; i++) {
            const GridSpan q = quads.at(i);
            hipLaunchKernelGGL(ksk_pack_kernel, dim3((osz + 255) / 256, q.count), dim3(256), 0, stream, d_ksk_std.ptr + q.first * 4 * osz,
                               d_ksk_packed.ptr + q.first * 8 * osz, (uint32_t)(rows - q.first * 4), osz);
        }
        const uint32_t tiles = (p.k * p.N + KS_IC - 1) / KS_IC, tile_rows = (uint32_t)KS_IC * p.ks_level;
        if (d_ksk_rowsum.alloc((size_t)tiles * osz * 8)) return 1;
        const GridSpans tsp = spans(tiles, 1);
        for (uint64_t i = 0; i < tsp.spans; i++) {
            const GridSpan t = tsp.at(i);
            hipLaunchKernelGGL(ksk_rowsum_kernel, dim3((osz + 255) / 256, t.count), dim3(256), 0, stream, d_ksk_std.ptr + t.first * tile_rows * osz,
                               d_ksk_rowsum.ptr + t.first * osz, (uint32_t)(rows - t.first * tile_rows), osz, tile_rows);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    d_ksk_mfma.release();
    // balanced base-256 digit planes in MFMA fragment order (ks_mfma_kernels.hip.h); a 16-slot group holds whole mask
    // elements with all their levels, so more than 16 levels (PARAM_MESSAGE_3_CARRY_4_COMPACT_PK_PBS_KS: 22) stay on the
    // byte-plane dot4 kernel
    if (cfg.ks_mfma_enabled && ks_mfma_supported(p.ks_level)) {
        const KsMfmaGeom g = ks_mfma_geom(p.k * p.N, p.n + 1, p.ks_level, p.ks_base_log);
        const size_t bytes = (size_t)g.col_groups * g.steps * 8 * 1024;
        if (d_ksk_mfma.alloc(bytes)) return 1;
        ks_mfma_repack(*this, d_ksk_std, d_ksk_mfma, g, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (d_fbsk.alloc(bsk_len * 8)) return 1;   // N u64 -> N/2 c64: same byte count
    if (convert_polys(d_std, d_fbsk, (uint32_t)(bsk_len / p.N))) return 1;
    if (convert_dense_key(d_std, (uint32_t)(bsk_len / p.N))) return 1;
    if (variant->combine_generic && probe_slot_exponents()) return 1;
    return allow_rotate_lds();
}

// fill_accumulator: shortint/engine/mod.rs:72-128.  box_values[i] = the torus value the table returns on box i
void fill_accumulator_torus(const fhe_params_t& p, const uint64_t* box_values, std::vector<uint64_t>& acc) {
    const uint32_t N = p.N, k = p.k;
    acc.assign((size_t)(k + 1) * N, 0);
    uint64_t* body = acc.data() + (size_t)k * N;
    const uint32_t modulus_sup = p.msg_mod * p.carry_mod;
    const uint32_t box = N / modulus_sup;
    std::vector<uint64_t> tmp(N);
    for (uint32_t i = 0; i < modulus_sup; i++)
        for (uint32_t j = 0; j < box; j++) tmp[(size_t)i * box + j] = box_values[i];
    const uint32_t half = box / 2;
    for (uint32_t j = 0; j < half; j++) tmp[j] = 0 - tmp[j];
    for (uint32_t j = 0; j < N; j++) body[j] = tmp[(j + half) % N];   // rotate_left(half)
}

uint64_t fill_accumulator(const fhe_params_t& p, const uint64_t* table, std::vector<uint64_t>& acc) {
    const uint32_t modulus_sup = p.msg_mod * p.carry_mod;
    const uint64_t delta = (1ull << 63) / modulus_sup;
    uint64_t maxv = 0;
    std::vector<uint64_t> values(modulus_sup);
    for (uint32_t i = 0; i < modulus_sup; i++) {
        maxv = table[i] > maxv ? table[i] : maxv;
        values[i] = table[i] * delta;
    }
    fill_accumulator_torus(p, values.data(), acc);
    return maxv;
}

int Engine::lut_upload(const uint64_t* acc, uint32_t* id) {
    if (use()) return 1;
    const size_t glwe = (size_t)(p.k + 1) * p.N;
    if ((size_t)(n_luts + 1) * glwe * 8 > d_luts.bytes) {      // grow and copy: the tables uploaded so far keep their ids
        DeviceBuffer<uint64_t> nl;
        if (nl.alloc(d_luts.bytes ? d_luts.bytes * 2 : 64 * glwe * 8)) return 1;
        if (d_luts) {
            if (sync_all_streams()) return 1;      // pipelined calls on the other streams may still read the old table array
            HIP_TRY(hipMemcpy(nl, d_luts, (size_t)n_luts * glwe * 8, hipMemcpyDeviceToDevice));
        }
        d_luts = std::move(nl);
    }
    HIP_TRY(hipMemcpyAsync(d_luts + (size_t)n_luts * glwe, acc, glwe * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *id = n_luts++;
    return 0;
}

int Engine::lut_download(uint32_t id, uint64_t* acc) {
    if (use()) return 1;
    if (id >= n_luts) return fail("bad LUT id");
    const size_t glwe = (size_t)(p.k + 1) * p.N;
    HIP_TRY(hipMemcpyAsync(acc, d_luts + (size_t)id * glwe, glwe * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int Engine::ensure_batch(uint32_t count) {
    const size_t big = (size_t)p.k * p.N + 1, small = (size_t)p.n + 1;
    return d_in.reserve(count * big * 8) || d_out.reserve(count * big * 8) || reserve_idle(pipe.lane[0].small, count * small * 8) || d_idx.reserve((size_t)count * 4);
}

// ---- matrix-core keyswitch: the host pieces its two users share (launch_keyswitch, Packing::pack_dev; ks_mfma_launch.h) ----
KsMfmaLaunch ks_mfma_plan(const KsMfmaGeom& g, uint32_t count, uint32_t base_log, int cu_count, uint32_t chunks_override) {
    KsMfmaLaunch l{};
    l.row_tiles = (count + 31) / 32;
    l.digit_bytes = (size_t)l.row_tiles * g.steps * 1024;
    l.mt = 1;
    while (l.mt < 8 && l.mt < l.row_tiles) l.mt *= 2;
    l.gy = (l.row_tiles + l.mt - 1) / l.mt;
    // K split over workgroups: enough waves to fill the 1024 SIMDs about one and a half times, no more -- every extra
    // chunk adds batch x columns 64-bit atomics (measured at 256 LWEs: 8 chunks 55 us, 32 chunks 89 us for memset +
    // digits + product; scripts/ks_bench.py; the packing product: up to 63 atomics per (tile, column group) and chunk)
    uint32_t chunks = (6u * (uint32_t)cu_count + g.col_groups * l.gy * l.mt / 2) / (g.col_groups * l.gy * l.mt);
    if (chunks_override) chunks = chunks_override;      // FHESTR_KS_CHUNKS
    chunks = std::max(1u, std::min(chunks, (g.steps + 7) / 8));
    chunks = std::max(chunks, (g.steps + ks_mfma_max_steps(base_log) - 1) / ks_mfma_max_steps(base_log));   // int32 accumulators
    l.spc = (g.steps + chunks - 1) / chunks;
    l.chunks = (g.steps + l.spc - 1) / l.spc;
    return l;
}
int ks_mfma_reserve_digits(Engine& e, DeviceBuffer<int8_t>& digits, const KsMfmaLaunch& l, hipStream_t s) {
    if (digits.bytes < l.digit_bytes) {
        if (e.reserve_idle(digits, l.digit_bytes)) return 1;
        HIP_TRY(hipMemsetAsync(digits, 0, l.digit_bytes, s));
    }
    return 0;
}
int ks_mfma_digits(Engine& e, DeviceBuffer<int8_t>& digits, const KsMfmaLaunch& l, const KsMfmaGeom& g, const uint64_t* d_lwes, uint32_t count, hipStream_t s) {
    if (ks_mfma_reserve_digits(e, digits, l, s)) return 1;
    // grid.y = samples: one launch per span of the device's grid.y, the span's first sample in the arguments
    const GridSpans sp = e.spans(count, 1);
    if (!sp.spans) return fail("keyswitch digits: the device reports no grid.y");
    for (uint64_t i = 0; i < sp.spans; i++) {
        const GridSpan b = sp.at(i);
        KsDecomposeArgs da{d_lwes, digits, g, count, (uint32_t)b.first};
        hipLaunchKernelGGL(ks_decompose_kernel, dim3((2 * g.steps + 255) / 256, b.count), dim3(256), 0, s, da);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
void ks_mfma_repack(const Engine& e, const uint64_t* d_std, int8_t* planes, const KsMfmaGeom& g, hipStream_t s) {
    const GridSpans sp = e.spans(g.steps, 1);      // grid.y = K steps of the key: 16384 at N = 32768 with 11 levels
    for (uint64_t i = 0; i < sp.spans; i++) {
        const GridSpan t = sp.at(i);
        hipLaunchKernelGGL(ksk_repack_mfma_kernel, dim3(g.col_groups, t.count), dim3(64), 0, s, d_std, planes, g, (uint32_t)t.first);
    }
}
int ks_mfma_product(const Engine& e, const KsMfmaArgs& ma, const KsMfmaLaunch& l, hipStream_t s) {
    // grid.y = row tiles / mt, at most 2048 under the 524280-LWE limit; grid.z = K chunks, at most steps / 8
    if (e.one_span("keyswitch product", l.gy, 1) || e.one_span("keyswitch product", l.chunks, 2)) return 1;
    switch (l.mt) {
        case 1: hipLaunchKernelGGL(keyswitch_mfma_kernel<1>, l.grid(ma.g), dim3(64), 0, s, ma); break;
        case 2: hipLaunchKernelGGL(keyswitch_mfma_kernel<2>, l.grid(ma.g), dim3(128), 0, s, ma); break;
        case 4: hipLaunchKernelGGL(keyswitch_mfma_kernel<4>, l.grid(ma.g), dim3(256), 0, s, ma); break;
        default: hipLaunchKernelGGL(keyswitch_mfma_kernel<8>, l.grid(ma.g), dim3(512), 0, s, ma); break;
    }
    return 0;
}

int Engine::launch_keyswitch(const uint64_t* d_big, uint64_t* d_sm, uint32_t count, DeviceBuffer<int8_t>& digits, hipStream_t on, bool shadow) {
    if (!d_ksk_packed) return fail("keys not loaded");
    hipStream_t s = on ? on : stream;
    // The documented batch limit (include/fhestr.h).  It was sized for the byte-plane kernel's grid.y = count / 8 under a cap
    // of 65535; what the device allows is hipDeviceProp_t::maxGridSize (max_grid), and every launch below is held to that.
    if (count > 65535u * KSD_S) return fail("batch too large for one keyswitch launch (max 524280 LWEs)");
    const uint32_t in_dim = p.k * p.N, out_size = p.n + 1;
    HIP_TRY(hipMemsetAsync(d_sm, 0, (size_t)count * out_size * 8, s));
    if (d_ksk_mfma && !shadow) {
        const KsMfmaGeom g = ks_mfma_geom(in_dim, out_size, p.ks_level, p.ks_base_log);
        const KsMfmaLaunch l = ks_mfma_plan(g, count, p.ks_base_log, cu_count, cfg.ks_chunks_override);
        if (ks_mfma_digits(*this, digits, l, g, d_big, count, s)) return 1;
        if (ks_mfma_product(*this, KsMfmaArgs{d_big + in_dim, in_dim + 1, d_ksk_mfma, digits, d_sm, g, count, l.row_tiles, l.spc}, l, s)) return 1;
        l.info(ks_last, FHE_KS_KERNEL_MFMA, g);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    KeyswitchPackedArgs pa{d_big, d_ksk_packed, d_ksk_rowsum, d_sm, in_dim, out_size, p.ks_base_log, p.ks_level, count};
    if (shadow) {     // small-register variant: co-resident with the blind rotation of the previous batch
        constexpr int S = 4;
        dim3 pgrid((out_size + KS_COLS - 1) / KS_COLS, (count + S - 1) / S, (in_dim + KS_IC - 1) / KS_IC);
        if (one_span("keyswitch", pgrid.y, 1) || one_span("keyswitch", pgrid.z, 2)) return 1;   // at most one LWE per CU here
        hipLaunchKernelGGL((keyswitch_dot4_kernel<S, 8>), pgrid, dim3(KS_COLS), (size_t)KS_IC * p.ks_level * S, s, pa);
        ks_last[0] = FHE_KS_KERNEL_DOT4_SHADOW; ks_last[1] = S; ks_last[2] = pgrid.z; ks_last[3] = KS_IC; ks_last[4] = in_dim;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // grid.y = tiles of KSD_S samples (65535 at the batch limit), one launch per span of the device's grid.y on its own rows of
    // both arrays; grid.z = tiles of KS_IC mask elements (1024 at k N = 65536)
    const uint32_t gx = (out_size + KS_COLS - 1) / KS_COLS, gz = (in_dim + KS_IC - 1) / KS_IC;
    const GridSpans sp = spans((count + KSD_S - 1) / KSD_S, 1);
    if (!sp.spans) return fail("keyswitch: the device reports no grid.y");
    if (one_span("keyswitch", gz, 2)) return 1;
    for (uint64_t i = 0; i < sp.spans; i++) {
        const GridSpan t = sp.at(i);
        KeyswitchPackedArgs ta = pa;
        ta.lwe_in += t.first * KSD_S * (in_dim + 1);
        ta.lwe_out += t.first * KSD_S * out_size;
        ta.batch = (uint32_t)(count - t.first * KSD_S);
        hipLaunchKernelGGL((keyswitch_dot4_kernel<KSD_S, 2>), dim3(gx, t.count, gz), dim3(KS_COLS), (size_t)KS_IC * p.ks_level * KSD_S, s, ta);
    }
    ks_last[0] = FHE_KS_KERNEL_DOT4; ks_last[1] = KSD_S; ks_last[2] = gz; ks_last[3] = KS_IC; ks_last[4] = in_dim;
    HIP_TRY(hipGetLastError());
    return 0;
}

// The refresh of both unpack forms (packing_dev.hip) and of Transcipher::next: count rows at d_cts through one keyswitch +
// PBS with the identity table over the whole message-and-carry space, in place, on the engine's stream.
int Engine::refresh_rows_dev(uint64_t* d_cts, uint32_t count) {
    const uint32_t M = p.msg_mod * p.carry_mod;
    std::vector<uint64_t> table(M), acc;
    for (uint32_t x = 0; x < M; x++) table[x] = x;
    fill_accumulator(table.data(), acc);
    uint32_t id = 0;
    if (lut_upload_dedup(acc, &id)) return 1;
    if (reserve_idle(refresh_idx, (size_t)count * 4)) return 1;   // an earlier refresh may still read the smaller array
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)refresh_idx.ptr, (int)id, count, stream));
    return ks_pbs_dev(d_cts, refresh_idx, d_cts, count);   // the keyswitch has read every row before the rotation writes one
}

void Engine::keyswitch_info(uint32_t info[6]) const {
    for (int q = 0; q < 5; q++) info[q] = ks_last[q];
    info[5] = rotate_registers();
}

// HIP events on the launch stream: per-call kernel durations without host synchronisation.  The ring is created whole or not at all.
int Engine::timing_events(hipEvent_t*& e4) {
    constexpr size_t RING = 1024;
    if (ring.empty()) {
        std::vector<hipEvent_t> fresh(RING * 4, nullptr);
        hipError_t err = hipSuccess;
        for (auto& e : fresh) if (err == hipSuccess) err = hipEventCreate(&e);
        if (err != hipSuccess) for (auto& e : fresh) if (e) (void)hipEventDestroy(e);
        HIP_TRY(err);
        ring.swap(fresh);
    }
    e4 = &ring[(ring_used++ % RING) * 4];   // keyswitch start / end, blind rotation start / end
    return 0;
}

// One call on one lane and stream, the lane's small buffer large enough: the keyswitch into it, the blind rotation out of it, the call's timing events around them.
static int ks_pbs_on_lane(Engine& e, PipeLane& lane, hipStream_t s, bool two_per_cu, const uint64_t* d_big_in, const uint32_t* d_lut_idx,
                          uint64_t* d_big_out, uint32_t count, hipEvent_t* e4) {
    HIP_TRY(hipEventRecord(e4[0], s));
    if (e.launch_keyswitch(d_big_in, lane.small, count, lane.digits, s)) return 1;
    HIP_TRY(hipEventRecord(e4[1], s));
    HIP_TRY(hipEventRecord(e4[2], s));
    if (e.launch_blind_rotate(lane.small, d_lut_idx, d_big_out, count, s, two_per_cu)) return 1;
    HIP_TRY(hipEventRecord(e4[3], s));
    return 0;
}

// Overlapped batches (fhe_engine_set_pipeline(2)): consecutive calls alternate between pipe.width (2) lanes and
// run on the two-LWEs-per-CU kernel with time-sliced priorities (BlindRotateArgs::fair_shift), so two 256-LWE
// launches share every CU and progress at the same rate -- the pace of a 512-LWE launch (2.09 ms per call,
// 122 k PBS/s) although every batch has 256 LWEs; the price is each call's latency (4.1 ms).  Three streams
// measured slower (119 k): the third launch's keyswitch waits for idle CUs.  Same ordering rules as mode 1, plus
// write-after-write / write-after-read against the calls still in flight on the other streams.  Results are
// those of the large-batch kernel.
static int ks_pbs_overlapped(Engine& e, const uint64_t* d_big_in, const uint32_t* d_lut_idx, uint64_t* d_big_out, uint32_t count, hipEvent_t* e4) {
    Pipeline& pl = e.pipe;
    const int ns = pl.width, slot = (int)(pl.calls % (uint64_t)pl.width);
    if (pl.ensure(ns)) return 1;
    PipeLane& lane = pl.lane[slot];
    hipStream_t s = pl.stream_of(slot, e.stream);
    if (e.reserve_idle(lane.small, count * ((size_t)e.p.n + 1) * 8)) return 1;   // the lane's previous rotation may still read it
    const size_t bytes = (size_t)count * ((size_t)e.p.k * e.p.N + 1) * 8;
    const ByteRange in{(const char*)d_big_in, (const char*)d_big_in + bytes}, out{(const char*)d_big_out, (const char*)d_big_out + bytes};
    if (pl.calls == 0) HIP_TRY(hipEventRecord(pl.run_start, e.stream));       // what the engine stream held before this run
    if (pl.calls < (uint64_t)ns && slot != 0) HIP_TRY(hipStreamWaitEvent(s, pl.run_start, 0));
    if (pl.input_ready) {
        HIP_TRY(hipStreamWaitEvent(s, pl.input_ready, 0));
        pl.input_ready = nullptr;
    }
    for (int q = 0; q < ns; q++)         // every call of this run on the other streams, not only their latest
        if (q != slot && pl.lane[q].blocks(in, out)) HIP_TRY(hipStreamWaitEvent(s, pl.lane[q].done, 0));
    lane.remember(in, out);
    if (ks_pbs_on_lane(e, lane, s, true, d_big_in, d_lut_idx, d_big_out, count, e4)) return 1;
    HIP_TRY(hipEventRecord(lane.done, s));
    pl.calls++;
    return 0;
}

// Pipelined mode (fhe_engine_set_pipeline): the keyswitch of this call runs on a second stream, in a 64-VGPR
// variant whose waves fit next to the two 220-VGPR waves per SIMD of the blind rotation still running for the
// previous call, into the other of two small-ciphertext buffers.  Calls are independent unless this call's
// input overlaps the previous call's output (older outputs are ordered by the buffer hand-over below).
static int ks_pbs_shadow(Engine& e, const uint64_t* d_big_in, const uint32_t* d_lut_idx, uint64_t* d_big_out, uint32_t count, hipEvent_t* e4) {
    Pipeline& pl = e.pipe;
    if (pl.ensure(2)) return 1;
    const int slot = (int)(pl.calls & 1);
    hipStream_t ks_stream = pl.stream_of(1, e.stream);
    if (e.reserve_idle(pl.lane[slot].small, count * ((size_t)e.p.n + 1) * 8)) return 1;
    uint64_t* sm = pl.lane[slot].small;
    const size_t bytes = (size_t)count * ((size_t)e.p.k * e.p.N + 1) * 8;
    const ByteRange in{(const char*)d_big_in, (const char*)d_big_in + bytes};
    if (pl.calls == 0) {
        // first pipelined call after anything else: whatever the engine stream already holds -- a serial call's
        // keyswitch / blind rotation that still use lane 0's small buffer, uploads, a caller's kernels -- comes first
        HIP_TRY(hipEventRecord(pl.run_start, e.stream));
        HIP_TRY(hipStreamWaitEvent(ks_stream, pl.run_start, 0));
    }
    if (pl.input_ready) {       // fhe_engine_pipeline_input_event: the producer of this call's input
        HIP_TRY(hipStreamWaitEvent(ks_stream, pl.input_ready, 0));
        pl.input_ready = nullptr;
    }
    if (pl.calls >= 1 && overlap(in, pl.prev_out[slot ^ 1]))
        HIP_TRY(hipStreamWaitEvent(ks_stream, pl.rot_done[slot ^ 1], 0));              // chained: input = previous output
    if (pl.calls >= 2) HIP_TRY(hipStreamWaitEvent(ks_stream, pl.rot_done[slot], 0));    // blind rotation that read `sm` two calls ago
    HIP_TRY(hipEventRecord(e4[0], ks_stream));
    if (e.launch_keyswitch(d_big_in, sm, count, pl.lane[slot].digits, ks_stream, true)) return 1;
    HIP_TRY(hipEventRecord(e4[1], ks_stream));
    HIP_TRY(hipEventRecord(pl.ks_done[slot], ks_stream));
    HIP_TRY(hipStreamWaitEvent(e.stream, pl.ks_done[slot], 0));
    HIP_TRY(hipEventRecord(e4[2], e.stream));
    if (e.launch_blind_rotate(sm, d_lut_idx, d_big_out, count)) return 1;
    HIP_TRY(hipEventRecord(e4[3], e.stream));
    HIP_TRY(hipEventRecord(pl.rot_done[slot], e.stream));
    pl.prev_out[slot] = {(const char*)d_big_out, (const char*)d_big_out + bytes};
    pl.calls++;
    return 0;
}

static int ks_pbs_serial(Engine& e, const uint64_t* d_big_in, const uint32_t* d_lut_idx, uint64_t* d_big_out, uint32_t count, hipEvent_t* e4) {
    if (e.pipe.calls && e.pipe.wait_others()) return 1;   // a serial call after pipelined ones: the other streams must be done with the shared buffers
    e.pipe.end_run();
    e.pipe.input_ready = nullptr;         // serial calls are stream-ordered: nothing to wait for
    if (e.reserve_idle(e.pipe.lane[0].small, count * ((size_t)e.p.n + 1) * 8)) return 1;
    return ks_pbs_on_lane(e, e.pipe.lane[0], e.stream, false, d_big_in, d_lut_idx, d_big_out, count, e4);
}

int Engine::ks_pbs_dev(const uint64_t* d_big_in, const uint32_t* d_lut_idx, uint64_t* d_big_out, uint32_t count, bool allow_pipeline) {
    if (use()) return 1;
    if (count == 0) return 0;
    hipEvent_t* e4 = nullptr;
    if (timing_events(e4)) return 1;
    if (allow_pipeline && pipeline == 2 && overlapped_mode_eligible(*this, count))
        return ks_pbs_overlapped(*this, d_big_in, d_lut_idx, d_big_out, count, e4);
    if (allow_pipeline && pipeline == 1 && shadow_mode_eligible(*this, count) && shadow_keyswitch_fits())
        return ks_pbs_shadow(*this, d_big_in, d_lut_idx, d_big_out, count, e4);
    return ks_pbs_serial(*this, d_big_in, d_lut_idx, d_big_out, count, e4);
}

int Engine::check_lut_idx(const uint32_t* lut_idx, uint32_t count) const {
    if (n_luts == 0) return fail("no lookup table uploaded");
    if (lut_idx)
        for (uint32_t i = 0; i < count; i++)
            if (lut_idx[i] >= n_luts) return fail("lut_idx out of range");
    return 0;
}

int Engine::ks_pbs_host(const uint64_t* in, const uint32_t* lut_idx, uint64_t* out, uint32_t count) {
    if (use()) return 1;
    if (count == 0) return 0;
    if (check_lut_idx(lut_idx, count)) return 1;
    if (ensure_batch(count)) return 1;
    const size_t big = (size_t)p.k * p.N + 1;
    HIP_TRY(hipMemcpyAsync(d_in, in, count * big * 8, hipMemcpyHostToDevice, stream));
    if (lut_idx) HIP_TRY(hipMemcpyAsync(d_idx, lut_idx, (size_t)count * 4, hipMemcpyHostToDevice, stream));
    if (ks_pbs_dev(d_in, lut_idx ? d_idx : nullptr, d_out, count)) return 1;
    HIP_TRY(hipMemcpyAsync(out, d_out, count * big * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return multi_cu.check();
}

int Engine::keyswitch_host(const uint64_t* in, uint64_t* out_small, uint32_t count) {
    if (use()) return 1;
    if (count == 0) return 0;
    if (ensure_batch(count)) return 1;
    const size_t big = (size_t)p.k * p.N + 1, small = (size_t)p.n + 1;
    HIP_TRY(hipMemcpyAsync(d_in, in, count * big * 8, hipMemcpyHostToDevice, stream));
    PipeLane& lane = pipe.lane[0];
    if (launch_keyswitch(d_in, lane.small, count, lane.digits)) return 1;
    HIP_TRY(hipMemcpyAsync(out_small, lane.small, count * small * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int Engine::pbs_host(const uint64_t* in_small, const uint32_t* lut_idx, uint64_t* out, uint32_t count) {
    if (use()) return 1;
    if (count == 0) return 0;
    if (check_lut_idx(lut_idx, count)) return 1;
    if (ensure_batch(count)) return 1;
    const size_t big = (size_t)p.k * p.N + 1, small = (size_t)p.n + 1;
    uint64_t* d_small = pipe.lane[0].small;
    HIP_TRY(hipMemcpyAsync(d_small, in_small, count * small * 8, hipMemcpyHostToDevice, stream));
    if (lut_idx) HIP_TRY(hipMemcpyAsync(d_idx, lut_idx, (size_t)count * 4, hipMemcpyHostToDevice, stream));
    if (launch_blind_rotate(d_small, lut_idx ? d_idx : nullptr, d_out, count)) return 1;
    HIP_TRY(hipMemcpyAsync(out, d_out, count * big * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return multi_cu.check();
}

// Small-key order (programmable_bootstrap_keyswitch_assign, shortint/server_key/mod.rs:859-932):
// ciphertexts live under the small LWE key; bootstrap first, then keyswitch back.
int Engine::pbs_ks_host(const uint64_t* in_small, const uint32_t* lut_idx, uint64_t* out_small, uint32_t count) {
    if (use()) return 1;
    if (count == 0) return 0;
    if (check_lut_idx(lut_idx, count)) return 1;
    // lane 1's small buffer is the second one here: a mode-2 call may still use it on its own stream
    if ((pipe.calls && pipe.wait_others()) || ensure_batch(count)) return 1;
    pipe.end_run();
    const size_t small = (size_t)p.n + 1;
    if (reserve_idle(pipe.lane[1].small, count * small * 8)) return 1;
    uint64_t *d_small = pipe.lane[0].small, *d_small2 = pipe.lane[1].small;
    HIP_TRY(hipMemcpyAsync(d_small, in_small, count * small * 8, hipMemcpyHostToDevice, stream));
    if (lut_idx) HIP_TRY(hipMemcpyAsync(d_idx, lut_idx, (size_t)count * 4, hipMemcpyHostToDevice, stream));
    if (launch_blind_rotate(d_small, lut_idx ? d_idx : nullptr, d_out, count)) return 1;
    if (launch_keyswitch(d_out, d_small2, count, pipe.lane[0].digits)) return 1;
    HIP_TRY(hipMemcpyAsync(out_small, d_small2, count * small * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return multi_cu.check();
}

int Engine::lincomb_dev(const uint64_t* d_pool_, const uint32_t* d_off, const uint32_t* d_src,
                        const int32_t* d_coeff, const uint64_t* d_cst, uint64_t* d_o, uint32_t jobs) {
    return lincomb_rows_dev(d_pool_, d_off, d_src, d_coeff, d_cst, d_o, jobs, p.k * p.N + 1);
}

int Engine::lincomb_rows_dev(const uint64_t* d_pool_, const uint32_t* d_off, const uint32_t* d_src, const int32_t* d_coeff, const uint64_t* d_cst,
                             uint64_t* d_o, uint32_t jobs, uint32_t row_words) {
    if (jobs == 0) return 0;
    LincombArgs a{d_pool_, d_off, d_src, d_coeff, d_cst, d_o, row_words, jobs};
    hipLaunchKernelGGL(lincomb_kernel, dim3(jobs), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int Engine::lincomb_batch_dev(const uint64_t* d_pool_, const uint32_t* d_off, const uint32_t* d_src, const int32_t* d_coeff,
                              const uint64_t* d_cst, uint64_t* d_o, uint32_t jobs, uint32_t instances, uint32_t src_slot, uint32_t src_inst,
                              uint32_t out_job, uint32_t out_inst, const uint32_t* d_lut_in, uint32_t* d_lut_out) {
    if (jobs == 0 || instances == 0) return 0;
    if ((uint64_t)jobs * instances > 0x7FFFFFFFull) return fail("lincomb batch: jobs * instances exceeds the grid limit");
    LincombBatchArgs b{{d_pool_, d_off, d_src, d_coeff, d_cst, d_o, p.k * p.N + 1, jobs}, instances, src_slot, src_inst, out_job, out_inst,
                       d_lut_in, d_lut_out};
    hipLaunchKernelGGL(lincomb_batch_kernel, dim3(jobs * instances), dim3(256), 0, stream, b);
    HIP_TRY(hipGetLastError());
    return 0;
}

int Engine::restride_dev(const uint64_t* d_i, uint64_t* d_o, uint32_t slots, uint32_t instances, uint32_t in_slot, uint32_t in_inst,
                         uint32_t out_slot, uint32_t out_inst) {
    if (slots == 0 || instances == 0) return 0;
    hipLaunchKernelGGL(lwe_restride_kernel, dim3(slots * instances), dim3(256), 0, stream, d_i, d_o, p.k * p.N + 1, instances, in_slot, in_inst,
                       out_slot, out_inst);
    HIP_TRY(hipGetLastError());
    return 0;
}

int Engine::lincomb_host(const uint64_t* pool, uint32_t pool_count, const uint32_t* off,
                         const uint32_t* src, const int32_t* coeff, const uint64_t* cst,
                         uint64_t* out, uint32_t jobs) {
    if (use()) return 1;
    if (jobs == 0) return 0;
    const size_t big = (size_t)p.k * p.N + 1;
    const uint32_t terms = off[jobs];
    for (uint32_t t = 0; t < terms; t++)
        if (src[t] >= pool_count) return fail("lincomb source index out of range");
    if (d_pool.reserve((size_t)pool_count * big * 8) || d_out.reserve((size_t)jobs * big * 8)) return 1;
    // meta: off | src | coeff | cst (8-byte aligned)
    const size_t o_off = 0, o_src = o_off + ((size_t)(jobs + 1) * 4 + 7) / 8 * 8;
    const size_t o_coeff = o_src + ((size_t)terms * 4 + 7) / 8 * 8;
    const size_t o_cst = o_coeff + ((size_t)terms * 4 + 7) / 8 * 8;
    const size_t meta_bytes = o_cst + (size_t)jobs * 8;
    if (d_meta.reserve(meta_bytes)) return 1;
    unsigned char* m = d_meta;
    HIP_TRY(hipMemcpyAsync(d_pool, pool, (size_t)pool_count * big * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(m + o_off, off, (size_t)(jobs + 1) * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(m + o_src, src, (size_t)terms * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(m + o_coeff, coeff, (size_t)terms * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(m + o_cst, cst, (size_t)jobs * 8, hipMemcpyHostToDevice, stream));
    if (lincomb_dev(d_pool, (const uint32_t*)(m + o_off), (const uint32_t*)(m + o_src),
                    (const int32_t*)(m + o_coeff), (const uint64_t*)(m + o_cst), d_out, jobs))
        return 1;
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)jobs * big * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int Engine::last_kernel_ms(float ms[2]) {
    if (use()) return 1;
    if (ring_used == 0) return fail("no ks_pbs call recorded");
    hipEvent_t* e4 = &ring[((ring_used - 1) % 1024) * 4];
    if (sync_all_streams()) return 1;
    HIP_TRY(hipEventSynchronize(e4[3]));
    HIP_TRY(hipEventElapsedTime(&ms[0], e4[0], e4[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], e4[2], e4[3]));
    return 0;
}

int Engine::kernel_times(double total_ms[2], uint32_t* calls, bool reset) {
    if (use()) return 1;
    if (sync_all_streams()) return 1;       // mode 2 records on every overlap stream
    const size_t nrec = ring_used < 1024 ? ring_used : 1024;
    total_ms[0] = total_ms[1] = 0.0;
    for (size_t c = 0; c < nrec; c++) {
        hipEvent_t* e4 = &ring[((ring_used - 1 - c) % 1024) * 4];
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e4[0], e4[1]));
        HIP_TRY(hipEventElapsedTime(&b, e4[2], e4[3]));
        total_ms[0] += a;
        total_ms[1] += b;
    }
    *calls = (uint32_t)nrec;
    if (reset) ring_used = 0;
    return 0;
}


int Engine::synchronize() {
    if (use()) return 1;
    if (sync_all_streams()) return 1;
    pipe.end_run();                       // every stream is idle: the next pipelined call starts a new run
    return multi_cu.check();
}

int Pipeline::ensure(int n) {
    if (n <= ready) return 0;
    hipError_t err = hipSuccess;
    for (int q = std::max(ready, 1); q < n && err == hipSuccess; q++) err = hipStreamCreateWithFlags(&lane[q].stream, hipStreamNonBlocking);
    if (!ready) each_event([&](hipEvent_t& e) { if (err == hipSuccess) err = hipEventCreateWithFlags(&e, hipEventDisableTiming); });
    if (err != hipSuccess) destroy(ready);     // all or nothing: what this call created goes, the next call tries again
    HIP_TRY(err);
    ready = n;
    return 0;
}

int Pipeline::wait_others() {
    for (int q = 1; q < ready; q++) HIP_TRY(hipStreamSynchronize(lane[q].stream));
    return 0;
}

int Pipeline::wait_all(hipStream_t engine) {
    if (wait_others()) return 1;
    HIP_TRY(hipStreamSynchronize(engine));
    return 0;
}

void Pipeline::end_run() {
    calls = 0;
    prev_out[0] = prev_out[1] = {nullptr, nullptr};
    for (auto& l : lane) { l.ins.clear(); l.outs.clear(); }
}

void Pipeline::destroy(int keep) {
    if (!keep) each_event([](hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; });
    for (int q = std::max(keep, 1); q < MAX_LANES; q++) {
        if (lane[q].stream) (void)hipStreamDestroy(lane[q].stream);
        lane[q].stream = nullptr;
    }
    ready = keep;
}


}  // namespace fhe
