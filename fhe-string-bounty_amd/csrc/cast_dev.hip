// cast_dev.hip -- fhe::CastKey (engine.h): the device side of casting keys (cast.h).  A cast is the matrix-core keyswitch
// at the cast key's geometry -- the digits by ks_decompose_kernel (LWE rows) or cast_decompose_glwe_kernel (packed GLWEs,
// cast_kernels.hip.h, instantiated here only), the product by keyswitch_mfma_kernel through ks_mfma_product -- and then
// what the target asks for: nothing, one ks_pbs level, or the blind rotation alone.  Everything is enqueued on the
// engine's stream; only the host forms, the first use of a follow-up table and a growing buffer synchronise.
//
// Floating-point contraction: off, as in engine.hip (-ffp-contract=off); no header included here turns it on.
#include "cast.h"
#include "cast_kernels.hip.h"
#include "engine.h"
#include "glwe_narrow.h"
#include "ks_mfma_launch.h"

namespace fhe {

static KsMfmaGeom geom_of(const CastKey& k) { return ks_mfma_geom(k.in_dim, k.out_size, k.cp.level, k.cp.base_log); }

// The words go up once and are rewritten into digit planes by the keyswitch's own ksk_repack_mfma_kernel; the 64-bit
// layout is released as soon as the planes exist (378 MB for PARAM_MESSAGE_1_CARRY_1 -> PARAM_MESSAGE_2_CARRY_2 TO_BIG).
int CastKey::create(Engine& e, const fhe_cast_params_t& cp, const uint64_t* words, CastKey** out) {
    *out = nullptr;
    if (e.use()) return 1;
    const std::string why = cast_params_check(e.p, cp);
    if (!why.empty()) return fail(why);
    const char* const who = "cast_key_create";
    std::unique_ptr<CastKey> k(new CastKey());
    k->e = &e;
    k->cp = cp;
    (void)cast_rshift(cp.src, e.p, &k->shift);
    k->in_dim = cast_in_dim(cp);
    k->out_size = cast_out_dim(e.p, cp) + 1;
    const KsMfmaGeom g = geom_of(*k);
    const size_t n_words = (size_t)cast_key_words(e.p, cp);
    DeviceBuffer<uint64_t> d_std;
    if (under(who, d_std.alloc(n_words * 8)) || under(who, k->key.alloc((size_t)g.col_groups * g.steps * 8 * 1024)) ||
        under(who, hipMemcpyAsync(d_std, words, n_words * 8, hipMemcpyHostToDevice, e.stream)))
        return 1;
    ks_mfma_repack(e, d_std, k->key, g, e.stream);
    if (under(who, hipGetLastError()) || under(who, hipStreamSynchronize(e.stream))) return 1;
    *out = k.get();
    e.cast_keys.push_back(std::move(k));
    return 0;
}

// Regrouping (widening casts of strings): `group` consecutive source blocks, the least significant first, become one
// destination block -- sum_i msg_src^i * row_i before the table x -> x >> shift.  The largest lookup input is
// (msg_src^group - 1) << shift and must stay inside the destination's message-and-carry space.
int CastKey::set_group(uint32_t new_group) {
    uint64_t degree, space;
    const std::string why = cast_regroup_check(cp.src, e->p, new_group, &degree, &space);
    if (!why.empty()) return fail(why);
    group = new_group;
    meta_count = 0;
    return 0;
}

int CastKey::gate(const char* who) const {
    double weight = 0, w = 1, v[3];                 // regrouping: variances add with the squared weights
    for (uint32_t i = 0; i < group; i++, w *= cp.src.msg_mod) weight += w * w;
    cast_noise_weighted(e->p, cp, v_in, weight, v);
    const double nu = v[0];
    if (nu <= v[1]) return 0;
    return fail(std::string(who) + ": refused, a block keyswitched under the cast pair (" + std::to_string(cp.base_log) + ", " + std::to_string(cp.level) +
                ") carries " + std::to_string(nu) + " nominal variances at the lookup that follows (source blocks declared at " + std::to_string(v_in) +
                "), the PBS-input budget is " + std::to_string(v[1]));
}

// memset, digits, product: count rows of out_size words at d_rows.  d_src: count LWE rows of in_dim + 1 words, or the
// source's packed GLWEs from the one that holds block 0.
int CastKey::keyswitch_dev(const uint64_t* d_src, uint32_t first, uint32_t count, bool packed, uint64_t* d_rows) {
    Engine& en = *e;
    if (count > 65535u) return fail("cast: batch too large for one launch (max 65535 blocks)");      // the documented limit (include/fhestr.h); the launches below are held to the device's maxGridSize
    const KsMfmaGeom g = geom_of(*this);
    const KsMfmaLaunch l = ks_mfma_plan(g, count, cp.base_log, en.cu_count, en.cfg.ks_chunks_override);
    hipStream_t s = en.stream;
    HIP_TRY(hipMemsetAsync(d_rows, 0, (size_t)count * out_size * 8, s));
    const uint64_t* d_bodies;
    uint32_t body_stride;
    if (packed && fused) {
        const uint32_t N = cp.src.N;
        if (N < 2 || (N & (N - 1))) return fail("cast_packed: the source polynomial size must be a power of two");
        if (ks_mfma_reserve_digits(en, digits, l, s) || en.reserve_idle(bodies, (size_t)count * 8)) return 1;
        CastDecomposeArgs a{d_src, digits, bodies, g, N, first, count, l.row_tiles};
        if (en.one_span("cast digits", l.row_tiles, 1)) return 1;      // grid.y = 32-row tiles: at most 2048 under the limit above
        hipLaunchKernelGGL(cast_decompose_glwe_kernel, dim3((g.steps + CAST_DECOMPOSE_WAVES - 1) / CAST_DECOMPOSE_WAVES, l.row_tiles),
                           dim3(64 * CAST_DECOMPOSE_WAVES), 0, s, a);
        d_bodies = bodies; body_stride = 1;
        last = 2;
    } else {
        const uint64_t* d_lwes = d_src;
        if (packed) {
            const uint32_t N = cp.src.N;
            if (N < 2 || (N & (N - 1))) return fail("cast_packed: the source polynomial size must be a power of two");
            if (en.reserve_idle(lwes, (size_t)count * (in_dim + 1) * 8)) return 1;
            if (en.packing.extract_dev("cast_packed", cp.src.k, N, d_src, first, count, lwes)) return 1;
            d_lwes = lwes;
        }
        if (ks_mfma_digits(en, digits, l, g, d_lwes, count, s)) return 1;
        d_bodies = d_lwes + in_dim; body_stride = in_dim + 1;
        last = packed ? 3 : 1;
    }
    if (ks_mfma_product(en, KsMfmaArgs{d_bodies, body_stride, key, digits, d_rows, g, count, l.row_tiles, l.spc}, l, s)) return 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

int CastKey::cast_dev(const uint64_t* d_src, uint32_t first, uint32_t count, bool packed, int mode, uint64_t* d_out) {
    Engine& en = *e;
    if (en.use()) return 1;
    if (mode != FHE_CAST_RAW && mode != FHE_CAST_REFRESH && mode != FHE_CAST_KEYSWITCHED) return fail("cast: unknown mode");
    if (count == 0) return 0;
    if (count % group) return fail("cast: " + std::to_string(count) + " blocks are not whole groups of " + std::to_string(group));
    const bool small = cp.target == FHE_CAST_TO_SMALL;
    const bool table = mode != FHE_CAST_KEYSWITCHED && (small || shift > 0 || mode == FHE_CAST_REFRESH);
    if (group > 1 && !table) return fail("cast: regrouped blocks need the shift table that follows");
    if (table && gate(packed ? "cast_packed" : "cast_lwes")) return 1;
    if (en.leave_pipelined_run()) return 1;                 // pipelined calls may still read or write these buffers on other streams
    if (!table) return keyswitch_dev(d_src, first, count, packed, d_out);      // the keyswitched rows are the result

    if (!en.d_fbsk) return fail("keys not loaded");
    const uint32_t n_out = count / group;
    if (en.reserve_idle(rows, (size_t)(count + (group > 1 ? n_out : 0)) * out_size * 8)) return 1;
    if (keyswitch_dev(d_src, first, count, packed, rows)) return 1;
    uint64_t* d_in = rows;
    if (group > 1) {       // row j = sum_i msg_src^i * row (j group + i): lincomb_kernel on rows of out_size words
        const size_t o_src = ((size_t)(n_out + 1) * 4 + 7) / 8 * 8, o_coeff = o_src + (size_t)count * 4, o_cst = (o_coeff + (size_t)count * 4 + 7) / 8 * 8;
        if (meta_count != count) {      // the lists depend on (count, group) alone; an earlier cast may still read the old ones
            std::vector<unsigned char> host(o_cst + (size_t)n_out * 8, 0);
            uint32_t* off = reinterpret_cast<uint32_t*>(host.data());
            uint32_t* src = reinterpret_cast<uint32_t*>(host.data() + o_src);
            int32_t* coeff = reinterpret_cast<int32_t*>(host.data() + o_coeff);
            for (uint32_t j = 0; j <= n_out; j++) off[j] = j * group;
            for (uint32_t t = 0; t < count; t++) {
                src[t] = t;
                int32_t w = 1;
                for (uint32_t i = 0; i < t % group; i++) w *= (int32_t)cp.src.msg_mod;
                coeff[t] = w;
            }
            if (en.sync_all_streams() || meta.reserve(host.size())) return 1;
            HIP_TRY(hipMemcpyAsync(meta, host.data(), host.size(), hipMemcpyHostToDevice, en.stream));
            HIP_TRY(hipStreamSynchronize(en.stream));
            meta_count = count;
        }
        unsigned char* m = meta;
        d_in = rows.ptr + (size_t)count * out_size;
        if (en.lincomb_rows_dev(rows, reinterpret_cast<const uint32_t*>(m), reinterpret_cast<const uint32_t*>(m + o_src), reinterpret_cast<const int32_t*>(m + o_coeff),
                           reinterpret_cast<const uint64_t*>(m + o_cst), d_in, n_out, out_size))
            return 1;
    }
    if (!lut_ready) {      // the follow-up table goes up once per key (the engine keeps tables for its lifetime)
        std::vector<uint64_t> values(e->p.msg_mod * e->p.carry_mod), acc;
        cast_shift_table(en.p, shift, values.data());
        en.fill_accumulator(values.data(), acc);
        if (en.lut_upload_dedup(acc, &lut)) return 1;
        lut_ready = true;
    }
    const uint32_t id = lut;
    if (en.reserve_idle(idx, (size_t)n_out * 4)) return 1;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)idx.ptr, (int)id, n_out, en.stream));
    if (small) return en.launch_blind_rotate(d_in, idx, d_out, n_out);
    return en.ks_pbs_dev(d_in, idx, d_out, n_out);
}

// Host rows / GLWEs through the staging buffers; synchronises, and reports what the multi-CU kernels left in their status block.
int CastKey::cast_host(const uint64_t* src, uint32_t first, uint32_t count, bool packed, int mode, uint64_t* dst) {
    Engine& en = *e;
    if (en.use()) return 1;
    if (count == 0) return 0;
    const size_t big = (size_t)en.p.k * en.p.N + 1;
    const size_t glwe_len = (size_t)(cp.src.k + 1) * cp.src.N;
    const uint64_t g_lo = packed ? first / cp.src.N : 0, g_hi = packed ? ((uint64_t)first + count - 1) / cp.src.N : 0;
    const size_t in_words = packed ? (size_t)(g_hi - g_lo + 1) * glwe_len : (size_t)count * (in_dim + 1);
    const size_t out_words = mode == FHE_CAST_KEYSWITCHED ? (size_t)count * out_size
                             : (cp.target == FHE_CAST_TO_BIG && shift <= 0 && mode == FHE_CAST_RAW) ? (size_t)count * big : (size_t)(count / group) * big;
    if (en.reserve_idle(in, in_words * 8) || en.reserve_idle(out, out_words * 8)) return 1;
    HIP_TRY(hipMemcpyAsync(in, src + (size_t)g_lo * glwe_len, in_words * 8, hipMemcpyHostToDevice, en.stream));
    if (cast_dev(in, packed ? first % cp.src.N : 0, count, packed, mode, out)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, out, out_words * 8, hipMemcpyDeviceToHost, en.stream));
    HIP_TRY(hipStreamSynchronize(en.stream));
    return mode == FHE_CAST_KEYSWITCHED ? 0 : en.multi_cu.check();
}

// A source client's narrow list (glwe_narrow.h): glwe_widen_kernel at the source's (k, N) rebuilds the GLWEs the range touches in
// `glwes` on the engine's stream, then the blocks are cast as packed GLWEs.  The list starts at its stream 0.
int CastKey::cast_narrow_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* d_out) {
    Engine& en = *e;
    if (en.use()) return 1;
    if ((uint64_t)first + count > held)
        return fail("cast_narrow: blocks " + std::to_string(first) + " .. " + std::to_string((uint64_t)first + count) + " asked of a list that holds " + std::to_string(held));
    if (count == 0) return 0;
    const uint32_t k = cp.src.k, N = cp.src.N;
    if (N < 2 || (N & (N - 1))) return fail("cast_narrow: the source polynomial size must be a power of two");
    if (en.reserve_idle(glwes, (size_t)(((uint64_t)held + N - 1) / N) * (k + 1) * N * 8)) return 1;
    if (en.packing.widen_shape_dev("cast_narrow", k, N, d_narrow, held, bits, glwes)) return 1;
    return cast_dev(glwes, first, count, true, mode, d_out);
}

int CastKey::cast_narrow_host(const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* dst) {
    Engine& en = *e;
    if (en.use()) return 1;
    const size_t words = narrow_len(cp.src.N, cp.src.k, held, bits);
    if (count == 0 || !words || (uint64_t)first + count > held) return cast_narrow_dev(nullptr, held, bits, first, count, mode, nullptr);   // nothing to do, or the refusal
    const size_t big = (size_t)en.p.k * en.p.N + 1;
    const size_t out_words = mode == FHE_CAST_KEYSWITCHED ? (size_t)count * out_size : (size_t)(count / group) * big;
    if (en.reserve_idle(in, words * 8) || en.reserve_idle(out, out_words * 8)) return 1;
    HIP_TRY(hipMemcpyAsync(in, narrow, words * 8, hipMemcpyHostToDevice, en.stream));
    if (cast_narrow_dev(in, held, bits, first, count, mode, out)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, out, out_words * 8, hipMemcpyDeviceToHost, en.stream));
    HIP_TRY(hipStreamSynchronize(en.stream));
    return mode == FHE_CAST_KEYSWITCHED ? 0 : en.multi_cu.check();
}

// The digit fragments alone, host arrays: what tests compare byte for byte between the two digit kernels.
int CastKey::digits_host(const uint64_t* src, uint32_t first, uint32_t count, bool packed, int8_t* dst, size_t* bytes) {
    Engine& en = *e;
    if (en.use()) return 1;
    const KsMfmaGeom g = geom_of(*this);
    const KsMfmaLaunch l = ks_mfma_plan(g, count, cp.base_log, en.cu_count, en.cfg.ks_chunks_override);
    *bytes = l.digit_bytes;
    if (!dst || count == 0) return 0;
    const size_t glwe_len = (size_t)(cp.src.k + 1) * cp.src.N;
    const uint64_t g_lo = packed ? first / cp.src.N : 0, g_hi = packed ? ((uint64_t)first + count - 1) / cp.src.N : 0;
    const size_t in_words = packed ? (size_t)(g_hi - g_lo + 1) * glwe_len : (size_t)count * (in_dim + 1);
    if (en.leave_pipelined_run()) return 1;
    if (en.reserve_idle(in, in_words * 8) || en.reserve_idle(rows, (size_t)count * out_size * 8)) return 1;
    HIP_TRY(hipMemcpyAsync(in, src + (size_t)g_lo * glwe_len, in_words * 8, hipMemcpyHostToDevice, en.stream));
    if (keyswitch_dev(in, packed ? first % cp.src.N : 0, count, packed, rows)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, digits, l.digit_bytes, hipMemcpyDeviceToHost, en.stream));
    HIP_TRY(hipStreamSynchronize(en.stream));
    return 0;
}

void CastKey::info(uint32_t out[8]) const {
    const uint32_t v[8] = {cp.target, cp.base_log, cp.level, in_dim, out_size - 1, (uint32_t)(shift + 64), fused ? 1u : 0u, last};
    std::copy(v, v + 8, out);
}

}  // namespace fhe
