// packing_dev.hip -- fhe::Packing (engine.h): the packed-ciphertext family of the engine.  The packing keyswitch (LWEs ->
// GLWEs, packing_ks_kernels.hip.h), the packed inputs (GLWEs -> LWEs, glwe_extract_kernels.hip.h) and the narrow packed
// results (GLWEs <-> b-bit lists -> LWEs, glwe_narrow_kernels.hip.h): the resident packing key, every launch of the three
// kernel headers, the staging of the host forms and the fhe_engine_*_info records; and ring packing, the second route from
// LWEs to the same GLWEs (ring_packing.h, ring_packing_kernels.hip.h), with its own resident key.  packing_ks_mfma_kernel<MT> is
// instantiated here only; its operand kernels and launch plan are the keyswitch's, reached through ks_mfma_launch.h.  The
// refresh after an extraction is Engine::refresh_rows_dev.
//
// Floating-point contraction: off, as in engine.hip (-ffp-contract=off); no header included here turns it on.
#include "engine.h"
#include "ks_mfma_launch.h"
#include "packing_ks_kernels.hip.h"
#include "glwe_extract_kernels.hip.h"
#include "glwe_narrow_kernels.hip.h"
#include "ring_packing_kernels.hip.h"

namespace fhe {

// The four host forms: the words at src through the staging buffer `in`, the device form, and the words of the staging
// buffer `out` back to dst; synchronises, and after a refresh reports what the multi-CU kernels left in their status block.
// A staging buffer a launch in flight may still read only grows once every stream is idle.
template <class Dev>
static int staged(Engine& e, DeviceBuffer<uint64_t>& in, const uint64_t* src, size_t in_words, DeviceBuffer<uint64_t>& out, uint64_t* dst, size_t out_words,
                  int refresh, Dev dev) {
    if (e.reserve_idle(in, in_words * 8) || e.reserve_idle(out, out_words * 8)) return 1;
    HIP_TRY(hipMemcpyAsync(in, src, in_words * 8, hipMemcpyHostToDevice, e.stream));
    if (dev(in.ptr, out.ptr)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, out, out_words * 8, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return refresh ? e.multi_cu.check() : 0;
}

// The refresh gate of both unpack forms: the loaded key's decomposition decides whether a raw block -- extracted from a
// full GLWE (bits = 0: packing_unpack_noise) or from a list narrowed to `bits` (narrow_noise) -- is within the PBS-input budget.
static int refresh_gate(const Packing& pk, const char* who, uint32_t bits) {
    if (!pk.key && pk.ring_key) {           // only the ring key is loaded: its model judges (ring_packing.h)
        double v[3];
        if (bits) ring_narrow_noise(pk.e->p, pk.ring_pp, bits, v); else ring_packing_noise(pk.e->p, pk.ring_pp, v);
        if (v[0] <= v[1]) return 0;
        return fail(std::string(who) + ": refresh refused, a raw block extracted" + (bits ? " at " + std::to_string(bits) + " bits" : std::string()) +
                    " under the ring packing pair (" + std::to_string(pk.ring_pp.base_log) + ", " + std::to_string(pk.ring_pp.level) + ") carries " +
                    std::to_string(v[0]) + " nominal variances, the PBS-input budget is " + std::to_string(v[1]));
    }
    if (!pk.key) return fail(std::string(who) + ": the refresh needs the loaded packing key's decomposition to judge the blocks' noise; none is loaded");
    double v[3];
    if (bits) narrow_noise(pk.e->p, pk.pp, bits, v); else packing_unpack_noise(pk.e->p, pk.pp, v);
    if (v[0] <= v[1]) return 0;
    const std::string block = !bits ? "extracted block" : "block extracted at " + std::to_string(bits) + " bits under the packing pair (" +
                                                              std::to_string(pk.pp.base_log) + ", " + std::to_string(pk.pp.level) + ")";
    return fail(std::string(who) + ": refresh refused, a raw " + block + " carries " + std::to_string(v[0]) + " nominal variances, the PBS-input budget is " +
                std::to_string(v[1]));
}

// The launch shape of both extraction kernels: count rows of kN + 1 words, GLWE_EXTRACT_PAIRS_PER_WG coefficient pairs per
// workgroup of 256 threads -> workgroups per row; the grid is count * chunks.
static int extract_chunks(const fhe_params_t& p, const char* who, uint32_t count, uint32_t* chunks) {
    *chunks = (p.k * p.N / 2 + GLWE_EXTRACT_PAIRS_PER_WG - 1) / GLWE_EXTRACT_PAIRS_PER_WG;
    if ((uint64_t)count * *chunks > 0x7FFFFFFFull) return fail(std::string(who) + ": too many ciphertexts for one launch");
    return 0;
}

// What the three narrow-family launches share: the grid limit, the record of the launch (fhe_engine_narrow_info) and the
// words of one GLWE's narrow stream, which their kernels take next to kN.
static int narrow_launch(Packing& pk, const char* who, uint32_t kernel, uint32_t bits, uint64_t items, uint64_t wgs, uint32_t* stride) {
    if (wgs > 0x7FFFFFFFull) return fail(std::string(who) + ": too many blocks for one launch");
    *stride = (uint32_t)narrow_stream_words((size_t)(pk.e->p.k + 1) * pk.e->p.N, bits);
    const uint32_t last[5] = {1, kernel, (uint32_t)items, (uint32_t)wgs, bits};
    std::copy(last, last + 5, pk.narrow_last);
    return 0;
}

// ---- packing keyswitch (packing_ks_kernels.hip.h) ---------------------------------------------------------------------
// The key [kN][level][k+1][N] goes up once and is rewritten into balanced base-256 digit planes by the keyswitch's own
// ksk_repack_mfma_kernel with (k+1) N columns; the 64-bit layout is then released.
int Packing::load_key(const fhe_packing_params_t& new_pp, const uint64_t* pksk) {
    if (e->use()) return 1;
    const fhe_params_t& p = e->p;
    if (packing_params_check(p, new_pp)) return 1;
    if (e->sync_all_streams()) return 1;                    // a launch in flight may still read the previous key or its digits
    const char* const who = "load_packing_key";
    key.release();
    digits.release();      // the pad slots depend on the level count
    for (auto& w : pack_last) w = 0;
    const KsMfmaGeom g = ks_mfma_geom(p.k * p.N, (p.k + 1) * p.N, new_pp.level, new_pp.base_log);
    const size_t words = (size_t)g.in_dim * new_pp.level * g.out_size;
    DeviceBuffer<uint64_t> d_std;
    DeviceBuffer<int8_t> planes;      // becomes the resident key only once it is complete
    if (d_std.alloc(words * 8)) return 1;
    if (under(who, planes.alloc((size_t)g.col_groups * g.steps * 8 * 1024)) ||
        under(who, hipMemcpyAsync(d_std, pksk, words * 8, hipMemcpyHostToDevice, e->stream)))
        return 1;
    ks_mfma_repack(*e, d_std, planes, g, e->stream);
    if (under(who, hipGetLastError()) || under(who, hipStreamSynchronize(e->stream))) return 1;
    d_std.release();      // the 64-bit layout (3.2 GB at N = 8192) goes as soon as the repack is done
    key = std::move(planes);
    pp = new_pp;
    return 0;
}

// count big-key LWEs at d_cts -> ceil(count / N) GLWEs at d_glwes: memset, digits, product with the rotate-and-sum
// epilogue.  Ordered on the engine's stream; nothing synchronises -- except in the throughput modes
// (fhe_engine_set_pipeline 1 / 2), whose calls write their outputs on other streams: there the call first waits for every
// stream and ends the pipelined run, like any serial call (include/fhestr.h says so).
int Packing::pack_dev(const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes) {
    if (e->use()) return 1;
    if (!key) return fail("packing key not loaded");
    if (count == 0) return 0;
    if (count > 65535u) return fail("batch too large for one packing launch (max 65535 LWEs)");   // the documented limit (include/fhestr.h); the launches below are held to the device's maxGridSize
    if (e->leave_pipelined_run()) return 1;                 // pipelined calls may still write the input on another stream
    const fhe_params_t& p = e->p;
    const uint32_t in_dim = p.k * p.N, out_size = (p.k + 1) * p.N;
    const KsMfmaGeom g = ks_mfma_geom(in_dim, out_size, pp.level, pp.base_log);
    const uint32_t n_glwe = (count + p.N - 1) / p.N;
    HIP_TRY(hipMemsetAsync(d_glwes, 0, (size_t)n_glwe * out_size * 8, e->stream));
    const KsMfmaLaunch l = ks_mfma_plan(g, count, pp.base_log, e->cu_count, e->cfg.ks_chunks_override);
    if (ks_mfma_digits(*e, digits, l, g, d_cts, count, e->stream)) return 1;
    PackKsArgs pa{d_cts, key, digits, d_glwes, g, count, l.row_tiles, l.spc, p.N, p.k * p.N / 32};
    if (e->one_span("packing product", l.gy, 1) || e->one_span("packing product", l.chunks, 2)) return 1;   // at most 256 row-tile groups; steps / 8 chunks
    switch (l.mt) {
        case 1: hipLaunchKernelGGL(packing_ks_mfma_kernel<1>, l.grid(g), dim3(64), 0, e->stream, pa); break;
        case 2: hipLaunchKernelGGL(packing_ks_mfma_kernel<2>, l.grid(g), dim3(128), 0, e->stream, pa); break;
        case 4: hipLaunchKernelGGL(packing_ks_mfma_kernel<4>, l.grid(g), dim3(256), 0, e->stream, pa); break;
        default: hipLaunchKernelGGL(packing_ks_mfma_kernel<8>, l.grid(g), dim3(512), 0, e->stream, pa); break;
    }
    l.info(pack_last, 1, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

int Packing::pack_host(const uint64_t* cts, uint32_t count, uint64_t* glwes) {
    if (e->use()) return 1;
    if (!key) return fail("packing key not loaded");
    if (count == 0) return 0;
    const fhe_params_t& p = e->p;
    const size_t big = (size_t)p.k * p.N + 1, out_words = (size_t)((count + p.N - 1) / p.N) * (p.k + 1) * p.N;
    return staged(*e, pack_in, cts, count * big, pack_out, glwes, out_words, 0,
                  [&](const uint64_t* d_cts, uint64_t* d_glwes) { return pack_dev(d_cts, count, d_glwes); });
}

// ---- packed inputs (glwe_extract_kernels.hip.h) -----------------------------------------------------------------------
// The extraction launch alone, at any GLWE shape (k, N), N a power of two: the engine's own set for unpack_dev, a source
// client's for a cast with the fused digit kernel off (CastKey::keyswitch_dev).  On the engine's stream.
int Packing::extract_dev(const char* who, uint32_t k, uint32_t N, const uint64_t* d_glwes, uint32_t first, uint32_t count, uint64_t* d_cts, uint32_t* chunks_out) {
    fhe_params_t shape = e->p;
    shape.k = k; shape.N = N;
    uint32_t chunks;
    if (extract_chunks(shape, who, count, &chunks)) return 1;
    hipLaunchKernelGGL(glwe_sample_extract_kernel, dim3(count * chunks), dim3(256), 0, e->stream, d_glwes, d_cts, N, k * N, first, count, chunks);
    HIP_TRY(hipGetLastError());
    if (chunks_out) *chunks_out = chunks;
    return 0;
}

// Blocks first .. first + count - 1 of the packed GLWEs at d_glwes (block j = coefficient j % N of GLWE j / N, the layout
// pack_dev writes) -> count big-key LWEs at d_cts.  Ordered on the engine's stream, nothing synchronises -- except,
// like pack_dev, in the throughput modes, and once per engine when the first refresh uploads the identity table.
// refresh: the extracted blocks carry the packing keyswitch's noise on top of a PBS output's, a plan's inputs are declared
// nominal (circuit.cpp: noise = 1.0); one ks_pbs level with the identity table over the whole message-and-carry space
// (Engine::refresh_rows_dev) brings them back, in place.  Refused where the model puts a raw block above the PBS-input budget.
int Packing::unpack_dev(const uint64_t* d_glwes, uint32_t first, uint32_t count, int refresh, uint64_t* d_cts) {
    if (e->use()) return 1;
    if (count == 0) return 0;
    const fhe_params_t& p = e->p;
    if (p.N < 2 || (p.N & (p.N - 1))) return fail("unpack_glwes: polynomial size must be a power of two");
    if (refresh && refresh_gate(*this, "unpack_glwes", 0)) return 1;
    if (e->leave_pipelined_run()) return 1;                 // pipelined calls may still read or write these buffers on other streams
    uint32_t chunks;
    if (extract_dev("unpack_glwes", p.k, p.N, d_glwes, first, count, d_cts, &chunks)) return 1;
    unpack_last[0] = 1; unpack_last[1] = count; unpack_last[2] = count * chunks; unpack_last[3] = 0;
    if (!refresh) return 0;
    if (e->refresh_rows_dev(d_cts, count)) return 1;
    unpack_last[3] = 1;
    return 0;
}

int Packing::unpack_host(const uint64_t* glwes, uint32_t first, uint32_t count, int refresh, uint64_t* cts) {
    if (e->use()) return 1;
    if (count == 0) return 0;
    const fhe_params_t& p = e->p;
    const size_t big = (size_t)p.k * p.N + 1, glwe_len = (size_t)(p.k + 1) * p.N;
    const uint64_t g_lo = first / p.N, g_hi = ((uint64_t)first + count - 1) / p.N;      // only the GLWEs the range touches go up
    return staged(*e, unpack_in, glwes + (size_t)g_lo * glwe_len, (size_t)(g_hi - g_lo + 1) * glwe_len, unpack_out, cts, count * big, refresh,
                  [&](const uint64_t* d_glwes, uint64_t* d_cts) { return unpack_dev(d_glwes, first % p.N, count, refresh, d_cts); });
}

// ---- narrow packed results (glwe_narrow.h, glwe_narrow_kernels.hip.h) -------------------------------------------------
// Both layout changes, one thread per word written: glwe_narrow_kernel (`words` of the list) or glwe_widen_kernel (of the
// GLWEs), at the GLWE shape (k, N): the engine's own, or a source client's for a cast (CastKey::cast_narrow_dev).
static int relayout(Packing& pk, const char* who, uint32_t kernel, uint32_t k, uint32_t N, const uint64_t* d_src, uint64_t* d_dst, uint32_t held, uint32_t bits,
                    uint64_t words) {
    Engine& e = *pk.e;
    if (e.leave_pipelined_run()) return 1;
    const uint64_t wgs = (words + 255) / 256;
    if (wgs > 0x7FFFFFFFull) return fail(std::string(who) + ": too many blocks for one launch");
    const uint32_t stride = (uint32_t)narrow_stream_words((size_t)(k + 1) * N, bits);
    const uint32_t last[5] = {1, kernel, (uint32_t)words, (uint32_t)wgs, bits};
    std::copy(last, last + 5, pk.narrow_last);
    hipLaunchKernelGGL(kernel == FHE_NARROW_KERNEL_NARROW ? glwe_narrow_kernel : glwe_widen_kernel, dim3((uint32_t)wgs), dim3(256), 0, e.stream, d_src, d_dst,
                       N, k * N, held, bits, stride, words);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The packed GLWEs of `held` blocks at d_glwes (what pack_dev wrote) -> their narrow list at d_narrow, narrow_len
// words.  Ordered on the engine's stream under pack_dev's contract.
int Packing::narrow_dev(const uint64_t* d_glwes, uint32_t held, uint32_t bits, uint64_t* d_narrow) {
    if (e->use()) return 1;
    const uint64_t words = narrow_len(e->p.N, e->p.k, held, bits);
    if (!words) return held ? fail("narrow_glwes: the width must be 8 .. 32 bits and the polynomial size a power of two") : 0;
    return relayout(*this, "narrow_glwes", FHE_NARROW_KERNEL_NARROW, e->p.k, e->p.N, d_glwes, d_narrow, held, bits, words);
}

// The inverse layout change on the device: the narrow list at d_narrow -> ceil(held / N) full GLWEs at d_glwes, what
// unpack_dev reads.  Same contract.
int Packing::widen_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint64_t* d_glwes) {
    return widen_shape_dev("widen_narrow", e->p.k, e->p.N, d_narrow, held, bits, d_glwes);
}

// The same at any GLWE shape (k, N): a source client's narrow list on the destination's engine.
int Packing::widen_shape_dev(const char* who, uint32_t k, uint32_t N, const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint64_t* d_glwes) {
    if (e->use()) return 1;
    if (!narrow_len(N, k, held, bits)) return held ? fail(std::string(who) + ": the width must be 8 .. 32 bits and the polynomial size a power of two") : 0;
    return relayout(*this, who, FHE_NARROW_KERNEL_WIDEN, k, N, d_narrow, d_glwes, held, bits, (((uint64_t)held + N - 1) / N) * ((uint64_t)(k + 1) * N));
}

int Packing::narrow_host(const uint64_t* glwes, uint32_t held, uint32_t bits, uint64_t* narrow) {
    if (e->use()) return 1;
    const fhe_params_t& p = e->p;
    const size_t words = narrow_len(p.N, p.k, held, bits), in_words = (size_t)(((uint64_t)held + p.N - 1) / p.N) * (p.k + 1) * p.N;
    if (!words) return narrow_dev(nullptr, held, bits, nullptr);      // nothing held, or the refusal
    return staged(*e, narrow_in, glwes, in_words, narrow_out, narrow, words, 0,
                  [&](const uint64_t* d_glwes, uint64_t* d_narrow) { return narrow_dev(d_glwes, held, bits, d_narrow); });
}

// Blocks first .. first + count - 1 of the narrow list of `held` blocks at d_narrow -> count big-key LWEs at d_cts: the
// rows unpack_dev would extract from the widened GLWEs, under its contract on streams and alignment.  The refresh is
// judged with the narrowing's term on top of the packing's (narrow_noise).
int Packing::unpack_narrow_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int refresh, uint64_t* d_cts) {
    if (e->use()) return 1;
    const fhe_params_t& p = e->p;
    if (!narrow_bits_ok(bits)) return fail("unpack_narrow: the width must be 8 .. 32 bits");
    if (!narrow_len(p.N, p.k, 1, bits)) return fail("unpack_narrow: polynomial size must be a power of two, (k + 1) N below 2^27");
    if ((uint64_t)first + count > held)
        return fail("unpack_narrow: blocks " + std::to_string(first) + " .. " + std::to_string((uint64_t)first + count) + " asked of a list that holds " + std::to_string(held));
    if (count == 0) return 0;
    if (refresh && refresh_gate(*this, "unpack_narrow", bits)) return 1;
    if (e->leave_pipelined_run()) return 1;
    uint32_t chunks, stride;
    if (extract_chunks(p, "unpack_narrow", count, &chunks) ||
        narrow_launch(*this, "unpack_narrow", FHE_NARROW_KERNEL_EXTRACT, bits, count, (uint64_t)count * chunks, &stride))
        return 1;
    hipLaunchKernelGGL(narrow_sample_extract_kernel, dim3(count * chunks), dim3(256), 0, e->stream, d_narrow, d_cts, p.N, p.k * p.N, held, bits, stride, first,
                       count, chunks);
    HIP_TRY(hipGetLastError());
    return refresh ? e->refresh_rows_dev(d_cts, count) : 0;
}

int Packing::unpack_narrow_host(const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int refresh, uint64_t* cts) {
    if (e->use()) return 1;
    const fhe_params_t& p = e->p;
    if (count == 0 || !narrow_len(p.N, p.k, held, bits) || (uint64_t)first + count > held)
        return unpack_narrow_dev(nullptr, held, bits, first, count, refresh, nullptr);   // nothing to do, or the refusal
    const size_t big = (size_t)p.k * p.N + 1, stride = narrow_stream_words((size_t)(p.k + 1) * p.N, bits);
    const uint32_t g_lo = first / p.N, g_hi = (first + count - 1) / p.N;     // only the streams the range touches go up
    const uint32_t held_up = std::min<uint64_t>(held, ((uint64_t)g_hi + 1) * p.N) - g_lo * p.N;   // a list of its own: streams g_lo .. g_hi
    return staged(*e, narrow_in, narrow + (size_t)g_lo * stride, narrow_len(p.N, p.k, held_up, bits), unpack_out, cts, count * big, refresh,
                  [&](const uint64_t* d_narrow, uint64_t* d_cts) { return unpack_narrow_dev(d_narrow, held_up, bits, first - g_lo * p.N, count, refresh, d_cts); });
}

// ---- ring packing (ring_packing.h, ring_packing_kernels.hip.h) --------------------------------------------------------
// Scratch is bounded.  The leaves and the nodes that replace them take count (k+1) N words: at most RING_SLOTS_CAP bytes,
// a longer list is refused (4,096 LWEs at N = 32768, k = 1).  A level's merges run in batches of at most RING_TMP_CAP bytes
// of transformed digits and lifted products (2.7 MB per merge at N = 32768 with five levels), whatever the list's length.
constexpr size_t RING_SLOTS_CAP = 2ull << 30, RING_TMP_CAP = 256ull << 20;

static uint32_t ring_threads(uint32_t N) { return std::min(RING_THREADS_MAX, N / 2); }

template <class K>
static int ring_allow_lds(K kernel, uint32_t N) {
    HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(N * 4)));
    return 0;
}

// N forward twiddles, then N inverse ones, at `tw`; ordered on `stream`, which the caller waits for while `tb` lives.
static int ring_upload_tables(const RingTables& tb, DeviceBuffer<uint32_t>& tw, hipStream_t stream) {
    if (tw.alloc((size_t)tb.N * 8)) return 1;
    HIP_TRY(hipMemcpyAsync(tw.ptr, tb.fwd.data(), (size_t)tb.N * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(tw.ptr + tb.N, tb.inv.data(), (size_t)tb.N * 4, hipMemcpyHostToDevice, stream));
    return 0;
}

// The key [log2 N][k][level][k+1][N] goes up once, every polynomial is rewritten into its eight transformed digit planes,
// and the 64-bit form is released.  A matrix packing key stays as it is.
int Packing::load_ring_key(const fhe_packing_params_t& new_pp, const uint64_t* key64) {
    if (e->use()) return 1;
    const fhe_params_t& p = e->p;
    const std::string why = ring_packing_check(p, new_pp);
    if (!why.empty()) return fail(why);
    if (e->sync_all_streams()) return 1;                    // a launch in flight may still read the previous key
    const char* const who = "load_ring_packing_key";
    ring_key.release();
    for (auto& w : ring_last) w = 0;
    const uint32_t N = p.N, logN = ring_log2(N);
    const size_t words = (size_t)ring_packing_key_words(p, new_pp), rows = words / N;
    RingTables tb;
    ring_tables(N, &tb);
    DeviceBuffer<uint64_t> d_std;
    DeviceBuffer<uint32_t> planes;      // becomes the resident key only once it is complete
    if (under(who, d_std.alloc(words * 8)) || under(who, planes.alloc(words * RING_PLANES * 4)) || under(who, ring_upload_tables(tb, ring_tw, e->stream)) ||
        under(who, hipMemcpyAsync(d_std, key64, words * 8, hipMemcpyHostToDevice, e->stream)))
        return 1;
    if (ring_allow_lds(ring_key_planes_kernel, N) || ring_allow_lds(ring_digits_kernel, N) || ring_allow_lds(ring_mac_kernel, N)) return 1;
    hipLaunchKernelGGL(ring_key_planes_kernel, dim3((uint32_t)rows, RING_PLANES), dim3(ring_threads(N)), N * 4, e->stream, d_std.ptr, planes.ptr, ring_tw.ptr, N, logN);
    if (under(who, hipGetLastError()) || under(who, hipStreamSynchronize(e->stream))) return 1;
    ring_key = std::move(planes);
    ring_pp = new_pp;
    ring_n_inv = tb.n_inv;
    return 0;
}

// count big-key LWEs at d_cts -> ceil(count / N) GLWEs at d_glwes in pack_dev's layout, under pack_dev's contract: ordered
// on the engine's stream, nothing synchronises except to leave a pipelined run and to grow the scratch.
int Packing::ring_pack_dev(const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes) {
    if (e->use()) return 1;
    if (!ring_key) return fail("ring packing key not loaded");
    if (count == 0) return 0;
    const fhe_params_t& p = e->p;
    const uint32_t N = p.N, k = p.k, k1 = k + 1, L = ring_pp.level, kL = k * L, logN = ring_log2(N);
    const size_t glwe_len = (size_t)k1 * N, slot_bytes = (size_t)count * glwe_len * 8;
    if (count > 65535u) return fail("batch too large for one ring packing call (max 65535 LWEs)");   // the documented limit (include/fhestr.h)
    if (slot_bytes > RING_SLOTS_CAP)
        return fail("ring packing: " + std::to_string(count) + " LWEs need " + std::to_string(slot_bytes) + " bytes of leaves, the cap is " +
                    std::to_string(RING_SLOTS_CAP) + "; pack the list in parts of whole GLWEs");
    if (e->leave_pipelined_run()) return 1;                 // pipelined calls may still write the input on another stream
    const uint32_t full_groups = count / N, c_last = count % N;
    const size_t per_merge = (size_t)N * 8 + (size_t)kL * N * 4 + (size_t)k1 * RING_PLANES * N * 4;
    const uint64_t widest = (uint64_t)full_groups * (N / 2) + std::min(N / 2, c_last);      // level 1
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({widest, RING_TMP_CAP / per_merge, 65535u, e->max_grid[2]}));   // merges per launch: grid.z of the combine kernel
    if (e->reserve_idle(ring_slots, slot_bytes) || e->reserve_idle(ring_tmp, batch * per_merge)) return 1;
    RingLevelArgs a{};
    a.slots = ring_slots;
    a.sigma_b = reinterpret_cast<uint64_t*>(ring_tmp.ptr);
    a.digits = reinterpret_cast<uint32_t*>(ring_tmp.ptr + (size_t)batch * N * 8);
    a.lifted = reinterpret_cast<int32_t*>(ring_tmp.ptr + (size_t)batch * N * 8 + (size_t)batch * kL * N * 4);
    a.fwd = ring_tw;
    a.inv = ring_tw.ptr + N;
    a.N = N; a.logN = logN; a.k = k; a.L = L; a.base_log = ring_pp.base_log; a.n_inv = ring_n_inv;
    a.full_groups = full_groups; a.c_last = c_last;
    // grid.y = LWEs: one launch per span of the device's grid.y, each on its own rows of both arrays
    const GridSpans leaves = e->spans(count, 1);
    if (!leaves.spans) return fail("ring packing: the device reports no grid.y");
    if (e->one_span("ring packing", batch, 2)) return 1;
    for (uint64_t i = 0; i < leaves.spans; i++) {
        const GridSpan lf = leaves.at(i);
        hipLaunchKernelGGL(ring_leaf_kernel, dim3((uint32_t)((glwe_len + 255) / 256), lf.count), dim3(256), 0, e->stream,
                           d_cts + lf.first * ((size_t)k * N + 1), ring_slots.ptr + lf.first * glwe_len, N, logN, k);
    }
    uint64_t launches = leaves.spans, keyswitches = 0;
    const uint32_t threads = ring_threads(N);
    for (uint32_t level = 1; level <= logN; level++) {
        a.s = N >> level;
        a.tinv = ring_tinv(N, level);
        a.key = ring_key.ptr + (size_t)(level - 1) * kL * k1 * RING_PLANES * N;
        a.final_out = level == logN ? d_glwes : nullptr;
        const uint32_t merges = full_groups * a.s + std::min(a.s, c_last);
        for (a.first = 0; a.first < merges; a.first += batch) {
            const uint32_t now = std::min(batch, merges - a.first);
            hipLaunchKernelGGL(ring_digits_kernel, dim3(now, kL + 1), dim3(threads), N * 4, e->stream, a);
            hipLaunchKernelGGL(ring_mac_kernel, dim3(now, k1 * RING_PLANES), dim3(threads), N * 4, e->stream, a);
            hipLaunchKernelGGL(ring_combine_kernel, dim3((N + 255) / 256, k1, now), dim3(256), 0, e->stream, a);
            launches += 3;
        }
        keyswitches += merges;
    }
    const uint64_t last[5] = {1, logN, keyswitches, launches, ring_slots.bytes + ring_tmp.bytes};
    std::copy(last, last + 5, ring_last);
    HIP_TRY(hipGetLastError());
    return 0;
}

int Packing::ring_pack_host(const uint64_t* cts, uint32_t count, uint64_t* glwes) {
    if (e->use()) return 1;
    if (!ring_key) return fail("ring packing key not loaded");
    if (count == 0) return 0;
    const fhe_params_t& p = e->p;
    const size_t big = (size_t)p.k * p.N + 1, out_words = (size_t)((count + p.N - 1) / p.N) * (p.k + 1) * p.N;
    return staged(*e, pack_in, cts, count * big, pack_out, glwes, out_words, 0,
                  [&](const uint64_t* d_cts, uint64_t* d_glwes) { return ring_pack_dev(d_cts, count, d_glwes); });
}

// The device transform on its own: count polynomials of N residues below P, host arrays, in place; synchronises.
int Packing::ring_ntt_host(uint32_t N, int inverse, uint32_t* polys, uint32_t count) {
    if (e->use()) return 1;
    if (N < RING_N_MIN || N > RING_N_MAX || (N & (N - 1))) return fail("ring transform: the size must be a power of two in 4 .. 32768");
    if (count == 0) return 0;
    for (size_t x = 0; x < (size_t)count * N; x++)
        if (polys[x] >= RING_P) return fail("ring transform: a residue is not below P");
    RingTables tb;
    ring_tables(N, &tb);
    DeviceBuffer<uint32_t> tw, d;
    if (ring_upload_tables(tb, tw, e->stream) || d.alloc((size_t)count * N * 4) || ring_allow_lds(ring_ntt_kernel, N)) return 1;
    HIP_TRY(hipMemcpyAsync(d.ptr, polys, (size_t)count * N * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(ring_ntt_kernel, dim3(count), dim3(ring_threads(N)), N * 4, e->stream, d.ptr, tw.ptr, tw.ptr + N, N, ring_log2(N), tb.n_inv, inverse);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(polys, d.ptr, (size_t)count * N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

}  // namespace fhe
