#include <algorithm>
// c_api.cpp -- extern "C" boundary (include/fhestr.h).  Mirrors the reference C API conventions:
// every entry point catches everything and returns 0/1 (c_api/utils.rs:3-12), out-pointers are
// nulled first so unchecked failures are loud (c_api/shortint/server_key/pbs.rs:24-29).
#include <exception>
#include <mutex>
#include <string>
#include <vector>

#include "det_math.h"
#include "engine.h"
#include "transcipher.h"

using fhe::fail;

#define API_BEGIN try {
#define API_END                                                   \
    }                                                             \
    catch (const std::exception& e) { return fail(e.what()); }    \
    catch (...) { return fail("unknown exception"); }

#define CHECK_PTR(p) \
    if (!(p)) return fail("null pointer: " #p)
// Calls on one engine from several host threads are serialised here (the reference's ServerKey is Sync: every thread
// brings its own scratch through a thread-local ShortintEngine, shortint/engine/mod.rs:23-25,184-189; this engine owns one
// set of staging buffers and one stream, so it takes a lock instead).  Recursive: fhe_str_* build plans through the
// same entry points.
#define LOCK_ENGINE(e) std::lock_guard<std::recursive_mutex> _engine_lock((e)->impl->mu)
#define LOCK_PLAN(p) \
    std::unique_lock<std::recursive_mutex> _plan_lock; \
    if ((p)->c->engine()) _plan_lock = std::unique_lock<std::recursive_mutex>((p)->c->engine()->mu)
// what an EngineSettings setter answered: nullptr (accepted), or why it refused the value and changed nothing
static int refused(const char* why) { return why ? fail(why) : 0; }

extern "C" {

const char* fhe_last_error(void) { return fhe::g_last_error.c_str(); }
const char* fhe_kernel_revision(void) { return FHESTR_KERNEL_REVISION; }

int fhe_engine_create(const fhe_params_t* params, int device, fhe_engine** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(params);
    fhe::Engine* e = nullptr;
    if (fhe::Engine::create(*params, device, &e)) return 1;
    *out = new fhe_engine{e, {}};
    return 0;
    API_END
}

int fhe_engine_destroy(fhe_engine* eng) {
    API_BEGIN
    if (!eng) return 0;
    for (auto& kv : eng->str_plans) fhe_plan_destroy(kv.second);
    delete eng->impl;
    delete eng;
    return 0;
    API_END
}

int fhe_engine_params(const fhe_engine* eng, fhe_params_t* out) {
    API_BEGIN
    CHECK_PTR(eng); CHECK_PTR(out);
    *out = eng->impl->p;
    return 0;
    API_END
}

int fhe_engine_load_keys(fhe_engine* eng, const uint64_t* bsk_std, const uint64_t* ksk) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(bsk_std); CHECK_PTR(ksk);
    return eng->impl->load_keys(bsk_std, ksk);
    API_END
}

int fhe_engine_generate_keys(fhe_engine* eng, const uint64_t* glwe_sk, const uint64_t* small_sk, const uint8_t seed[32],
                             uint64_t* bsk_std_out, uint64_t* ksk_out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(glwe_sk); CHECK_PTR(small_sk); CHECK_PTR(seed);
    return eng->impl->generate_keys(glwe_sk, small_sk, seed, bsk_std_out, ksk_out);
    API_END
}

void* fhe_engine_stream(fhe_engine* eng) { return eng ? (void*)eng->impl->stream : nullptr; }

int fhe_engine_synchronize(fhe_engine* eng) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return eng->impl->synchronize();
    API_END
}

int fhe_engine_set_variant(fhe_engine* eng, int log2_points) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return eng->impl->set_variant(log2_points);
    API_END
}

int fhe_engine_load_seeded_keys(fhe_engine* eng, const uint8_t ksk_seed[16], const uint64_t* ksk_bodies, const uint8_t bsk_seed[16],
                                const uint64_t* bsk_bodies, uint64_t* bsk_std_out, uint64_t* ksk_out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(ksk_seed); CHECK_PTR(ksk_bodies); CHECK_PTR(bsk_seed); CHECK_PTR(bsk_bodies);
    return eng->impl->load_seeded_keys(ksk_seed, ksk_bodies, bsk_seed, bsk_bodies, bsk_std_out, ksk_out);
    API_END
}

int fhe_engine_expand_seeded_lwe(fhe_engine* eng, const uint8_t* seeds, const uint64_t* bodies, uint32_t count, uint64_t* d_out,
                                 uint64_t* host_out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(seeds); CHECK_PTR(bodies); }
    if (!d_out && !host_out) return fhe::fail("expand_seeded_lwe: no destination");
    return eng->impl->expand_seeded_lwe(seeds, bodies, count, d_out, host_out);
    API_END
}

int fhe_engine_expand_compact_list(fhe_engine* eng, const uint64_t* list, uint32_t count, uint64_t* d_out, uint64_t* host_out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) CHECK_PTR(list);
    if (!d_out && !host_out) return fhe::fail("expand_compact_list: no destination");
    return eng->impl->expand_compact_list(list, count, d_out, host_out);
    API_END
}

int fhe_engine_expand_compact_list_dev(fhe_engine* eng, const uint64_t* d_list, uint32_t count, uint64_t* d_out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(d_list); CHECK_PTR(d_out); }
    return eng->impl->expand_compact_list_dev(d_list, count, d_out);
    API_END
}

int fhe_engine_set_pipeline(fhe_engine* eng, int on) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (eng->impl->synchronize()) return 1;
    if (on < 0 || on > 2) return fhe::fail("pipeline mode: 0 (off), 1 (keyswitch in the shadow of the previous blind rotation) or 2 (overlapped batches)");
    eng->impl->pipeline = on;
    return 0;
    API_END
}

int fhe_engine_pipeline_input_event(fhe_engine* eng, void* hip_event) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    eng->impl->pipe.input_ready = reinterpret_cast<hipEvent_t>(hip_event);
    return 0;
    API_END
}

// Not part of include/fhestr.h (tests only): the pipelined calls of the current run -- 0 again after any serial call or
// synchronisation -- so a test can tell that its calls took a throughput mode and none fell back to the serial path.
int fhe_debug_pipeline_calls(fhe_engine* eng) {
    if (!eng) return -1;
    LOCK_ENGINE(eng);
    return (int)eng->impl->pipe.calls;
}

// Not part of include/fhestr.h (tests only): the parts of the noise sampler (det_math.h) as the host compiles them, so the
// tests can hold them against a real logarithm and a real normal distribution (tests/test_exact_keys.py).
int fhe_debug_det_log(const double* x, size_t n, double* out) {
    if (n && (!x || !out)) return fail("null pointer");
    for (size_t i = 0; i < n; i++) out[i] = fhe::det_log(x[i]);
    return 0;
}

// `count` consecutive gaussian_torus values of one Rng (seed, stream)
int fhe_debug_noise_samples(const uint8_t seed[32], uint64_t stream, double std_dev, size_t count, uint64_t* out) {
    if (!seed || (count && !out)) return fail("null pointer");
    fhe::Rng r(fhe::seed_from_bytes(seed), stream);
    for (size_t i = 0; i < count; i++) out[i] = fhe::gaussian_torus(r, std_dev);
    return 0;
}

// round_half_away and from_torus_exact of every x
int fhe_debug_round_torus(const double* x, size_t n, double* rounded, uint64_t* torus) {
    if (n && (!x || !rounded || !torus)) return fail("null pointer");
    for (size_t i = 0; i < n; i++) {
        rounded[i] = fhe::round_half_away(x[i]);
        torus[i] = fhe::from_torus_exact(x[i]);
    }
    return 0;
}

int fhe_engine_set_multibit_combine_max(fhe_engine* eng, uint32_t max_batch) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return refused(eng->impl->cfg.set_multibit_combine_max(max_batch));
    API_END
}

int fhe_engine_set_cluster_mode(fhe_engine* eng, int mode, uint32_t max_batch) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return refused(eng->impl->cfg.set_cluster_mode(mode, max_batch));
    API_END
}

int fhe_engine_set_keep_busy(fhe_engine* eng, int on) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    eng->impl->cfg.set_keep_busy(on);
    return 0;
    API_END
}

int fhe_engine_cluster_info(fhe_engine* eng, uint32_t* clusters) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(clusters);
    if (eng->impl->synchronize()) return 1;
    *clusters = eng->impl->multi_cu.last_clusters();
    return 0;
    API_END
}

int fhe_engine_keyswitch_info(fhe_engine* eng, uint32_t info[6]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(info);
    if (eng->impl->use()) return 1;
    eng->impl->keyswitch_info(info);
    return 0;
    API_END
}

int fhe_engine_load_packing_key(fhe_engine* eng, const fhe_packing_params_t* pp, const uint64_t* pksk) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(pp); CHECK_PTR(pksk);
    return eng->impl->packing.load_key(*pp, pksk);
    API_END
}

int fhe_engine_pack_lwes(fhe_engine* eng, const uint64_t* cts, uint32_t count, uint64_t* glwes_host) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(cts); CHECK_PTR(glwes_host); }
    return eng->impl->packing.pack_host(cts, count, glwes_host);
    API_END
}

int fhe_engine_pack_lwes_dev(fhe_engine* eng, const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(d_cts); CHECK_PTR(d_glwes); }
    return eng->impl->packing.pack_dev(d_cts, count, d_glwes);
    API_END
}

int fhe_engine_packing_info(fhe_engine* eng, uint32_t info[5]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(info);
    eng->impl->packing.pack_info(info);
    return 0;
    API_END
}

int fhe_engine_load_ring_packing_key(fhe_engine* eng, const fhe_packing_params_t* pp, const uint64_t* key) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(pp); CHECK_PTR(key);
    return eng->impl->packing.load_ring_key(*pp, key);
    API_END
}

int fhe_engine_ring_pack_lwes(fhe_engine* eng, const uint64_t* cts, uint32_t count, uint64_t* glwes_host) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(cts); CHECK_PTR(glwes_host); }
    return eng->impl->packing.ring_pack_host(cts, count, glwes_host);
    API_END
}

int fhe_engine_ring_pack_lwes_dev(fhe_engine* eng, const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(d_cts); CHECK_PTR(d_glwes); }
    return eng->impl->packing.ring_pack_dev(d_cts, count, d_glwes);
    API_END
}

int fhe_engine_ring_pack_info(fhe_engine* eng, uint64_t info[5]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(info);
    std::copy(eng->impl->packing.ring_last, eng->impl->packing.ring_last + 5, info);
    return 0;
    API_END
}

int fhe_engine_ring_ntt(fhe_engine* eng, uint32_t N, int inverse, uint32_t* polys, uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) CHECK_PTR(polys);
    return eng->impl->packing.ring_ntt_host(N, inverse, polys, count);
    API_END
}

int fhe_engine_unpack_glwes(fhe_engine* eng, const uint64_t* glwes_host, uint32_t first, uint32_t count, int refresh, uint64_t* cts_host) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(glwes_host); CHECK_PTR(cts_host); }
    return eng->impl->packing.unpack_host(glwes_host, first, count, refresh, cts_host);
    API_END
}

int fhe_engine_unpack_glwes_dev(fhe_engine* eng, const uint64_t* d_glwes, uint32_t first, uint32_t count, int refresh, uint64_t* d_cts) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(d_glwes); CHECK_PTR(d_cts); }
    return eng->impl->packing.unpack_dev(d_glwes, first, count, refresh, d_cts);
    API_END
}

int fhe_engine_unpack_info(fhe_engine* eng, uint32_t info[4]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(info);
    eng->impl->packing.unpack_info(info);
    return 0;
    API_END
}

int fhe_engine_narrow_glwes(fhe_engine* eng, const uint64_t* glwes_host, uint32_t held, uint32_t bits, uint64_t* narrow_host) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (held) { CHECK_PTR(glwes_host); CHECK_PTR(narrow_host); }
    return eng->impl->packing.narrow_host(glwes_host, held, bits, narrow_host);
    API_END
}

int fhe_engine_narrow_glwes_dev(fhe_engine* eng, const uint64_t* d_glwes, uint32_t held, uint32_t bits, uint64_t* d_narrow) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (held) { CHECK_PTR(d_glwes); CHECK_PTR(d_narrow); }
    return eng->impl->packing.narrow_dev(d_glwes, held, bits, d_narrow);
    API_END
}

int fhe_engine_widen_narrow_dev(fhe_engine* eng, const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint64_t* d_glwes) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (held) { CHECK_PTR(d_narrow); CHECK_PTR(d_glwes); }
    return eng->impl->packing.widen_dev(d_narrow, held, bits, d_glwes);
    API_END
}

int fhe_engine_unpack_narrow(fhe_engine* eng, const uint64_t* narrow_host, uint32_t held, uint32_t bits, uint32_t first, uint32_t count,
                             int refresh, uint64_t* cts_host) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(narrow_host); CHECK_PTR(cts_host); }
    return eng->impl->packing.unpack_narrow_host(narrow_host, held, bits, first, count, refresh, cts_host);
    API_END
}

int fhe_engine_unpack_narrow_dev(fhe_engine* eng, const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count,
                                 int refresh, uint64_t* d_cts) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    if (count) { CHECK_PTR(d_narrow); CHECK_PTR(d_cts); }
    return eng->impl->packing.unpack_narrow_dev(d_narrow, held, bits, first, count, refresh, d_cts);
    API_END
}

int fhe_engine_narrow_info(fhe_engine* eng, uint32_t info[5]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(info);
    eng->impl->packing.narrow_info(info);
    return 0;
    API_END
}

int fhe_engine_cluster_fallbacks(fhe_engine* eng, uint32_t* count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(count);
    *count = eng->impl->multi_cu.fallbacks();
    return 0;
    API_END
}

int fhe_lut_generate(fhe_engine* eng, const uint64_t* table, uint32_t* lut_id, uint64_t* degree) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(table); CHECK_PTR(lut_id);
    std::vector<uint64_t> acc;
    uint64_t deg = eng->impl->fill_accumulator(table, acc);
    if (degree) *degree = deg;
    return eng->impl->lut_upload_dedup(acc, lut_id);
    API_END
}

int fhe_lut_upload(fhe_engine* eng, const uint64_t* accumulator, uint32_t* lut_id) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(accumulator); CHECK_PTR(lut_id);
    return eng->impl->lut_upload(accumulator, lut_id);
    API_END
}

int fhe_lut_download(fhe_engine* eng, uint32_t lut_id, uint64_t* accumulator) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(accumulator);
    return eng->impl->lut_download(lut_id, accumulator);
    API_END
}

int fhe_lut_count(const fhe_engine* eng, uint32_t* count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(count);
    *count = eng->impl->n_luts;
    return 0;
    API_END
}

int fhe_keyswitch_batch(fhe_engine* eng, const uint64_t* in, uint64_t* out, uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(in); CHECK_PTR(out);
    return eng->impl->keyswitch_host(in, out, count);
    API_END
}

int fhe_pbs_batch(fhe_engine* eng, const uint64_t* in, const uint32_t* lut_idx, uint64_t* out,
                  uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(in); CHECK_PTR(out);
    return eng->impl->pbs_host(in, lut_idx, out, count);
    API_END
}

int fhe_pbs_ks_batch(fhe_engine* eng, const uint64_t* in, const uint32_t* lut_idx, uint64_t* out,
                     uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(in); CHECK_PTR(out);
    return eng->impl->pbs_ks_host(in, lut_idx, out, count);
    API_END
}

int fhe_ks_pbs_batch(fhe_engine* eng, const uint64_t* in, const uint32_t* lut_idx, uint64_t* out,
                     uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(in); CHECK_PTR(out);
    return eng->impl->ks_pbs_host(in, lut_idx, out, count);
    API_END
}

int fhe_ks_pbs_batch_dev(fhe_engine* eng, const uint64_t* d_in, const uint32_t* d_lut_idx,
                         uint64_t* d_out, uint32_t count) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(d_in); CHECK_PTR(d_out);
    return eng->impl->ks_pbs_dev(d_in, d_lut_idx, d_out, count, /*allow_pipeline=*/true);
    API_END
}

int fhe_lwe_lincomb_batch(fhe_engine* eng, const uint64_t* pool, uint32_t pool_count,
                          const uint32_t* off, const uint32_t* src, const int32_t* coeff,
                          const uint64_t* cst, uint64_t* out, uint32_t jobs) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(pool); CHECK_PTR(off); CHECK_PTR(src); CHECK_PTR(coeff);
    CHECK_PTR(cst); CHECK_PTR(out);
    return eng->impl->lincomb_host(pool, pool_count, off, src, coeff, cst, out, jobs);
    API_END
}

int fhe_last_kernel_ms(fhe_engine* eng, float ms[2]) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(ms);
    return eng->impl->last_kernel_ms(ms);
    API_END
}

int fhe_kernel_times(fhe_engine* eng, double total_ms[2], uint32_t* calls, int reset) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(total_ms); CHECK_PTR(calls);
    return eng->impl->kernel_times(total_ms, calls, reset != 0);
    API_END
}

}  // extern "C"

// ---- plans: levelised shortint circuits + FheString operations ----------------------------------
#include "circuit.h"

namespace fhe {
int build_string_op(Circuit& c, const std::string& op, uint32_t a_cap, uint32_t b_cap,
                    const uint8_t* clear, uint32_t clear_len);
int build_integer_op(Circuit& c, const std::string& op, uint32_t n_blocks, uint64_t scalar);
}
#include "noise_model.h"
#include "regex.h"
#include "str_op_name.h"
#include "str_program.h"

struct fhe_plan {
    fhe::Circuit* c;
    bool finalized;
};

extern "C" {

int fhe_plan_create(fhe_engine* eng, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    *out = new fhe_plan{new fhe::Circuit(eng->impl->p, eng->impl), false};
    return 0;
    API_END
}

int fhe_plan_create_offline(const fhe_params_t* params, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(params);
    *out = new fhe_plan{new fhe::Circuit(*params, nullptr), false};
    return 0;
    API_END
}

int fhe_engine_set_stream(fhe_engine* eng, void* hip_stream) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return eng->impl->set_stream((hipStream_t)hip_stream, false);
    API_END
}

int fhe_engine_reset_stream(fhe_engine* eng) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    return eng->impl->set_stream(nullptr, true);
    API_END
}

int fhe_plan_destroy(fhe_plan* p) {
    API_BEGIN
    if (!p) return 0;
    {
        LOCK_PLAN(p);          // the circuit's destructor releases device memory of the engine's GPU
        delete p->c;
    }
    delete p;
    return 0;
    API_END
}

#define PLAN_BUILDING(p)                                   \
    CHECK_PTR(p);                                          \
    LOCK_PLAN(p);                                          \
    if ((p)->finalized) return fail("plan already finalised")
#define PLAN_READY(p)                                      \
    CHECK_PTR(p);                                          \
    LOCK_PLAN(p);                                          \
    if (!(p)->finalized) return fail("plan not finalised")

int fhe_plan_input(fhe_plan* p, uint64_t degree, uint32_t* node) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(node);
    *node = p->c->input(degree);
    return 0;
    API_END
}

int fhe_plan_lut(fhe_plan* p, const uint64_t* table, uint32_t* lut) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(table); CHECK_PTR(lut);
    std::vector<uint64_t> t(table, table + p->c->total_modulus());
    *lut = p->c->lut(t);
    if (p->c->failed()) return fail(p->c->take_error());
    return 0;
    API_END
}

int fhe_plan_lin(fhe_plan* p, const uint32_t* nodes, const int32_t* coeffs, uint32_t n_terms,
                 int64_t constant, uint32_t* node) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(node);
    if (n_terms) { CHECK_PTR(nodes); CHECK_PTR(coeffs); }
    std::vector<fhe::Term> terms;
    for (uint32_t i = 0; i < n_terms; i++) terms.push_back({nodes[i], coeffs[i]});
    *node = p->c->lin(terms, constant);
    if (p->c->failed()) return fail(p->c->take_error());
    return 0;
    API_END
}

int fhe_plan_pbs(fhe_plan* p, uint32_t src, uint32_t lut, uint32_t* node) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(node);
    *node = p->c->pbs(src, lut);
    if (p->c->failed()) return fail(p->c->take_error());
    return 0;
    API_END
}

int fhe_plan_pbs_signed(fhe_plan* p, uint32_t src, uint32_t lut, uint32_t* node) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(node);
    *node = p->c->pbs(src, lut, true);
    if (p->c->failed()) return fail(p->c->take_error());
    return 0;
    API_END
}

int fhe_plan_pbs_full_box(fhe_plan* p, uint32_t src, int all, uint32_t* node) {
    API_BEGIN
    PLAN_BUILDING(p); CHECK_PTR(node);
    *node = p->c->pbs_full_box(src, all != 0);
    if (p->c->failed()) return fail(p->c->take_error());
    return 0;
    API_END
}

int fhe_plan_set_owner_hint(fhe_plan* p, int rank) {
    API_BEGIN
    PLAN_BUILDING(p);
    p->c->set_owner_hint(rank);
    return 0;
    API_END
}

int fhe_plan_output(fhe_plan* p, uint32_t node) {
    API_BEGIN
    PLAN_BUILDING(p);
    p->c->output(node);
    return 0;
    API_END
}

int fhe_plan_finalize(fhe_plan* p, uint32_t world) {
    API_BEGIN
    PLAN_BUILDING(p);
    if (p->c->finalize(world)) return 1;
    p->finalized = true;
    return 0;
    API_END
}

static int str_plan(const fhe_params_t& params, fhe::Engine* eng, const char* op, uint32_t a_cap,
                    uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, uint32_t world, fhe_plan** out) {
    fhe::Circuit* c = new fhe::Circuit(params, eng);
    c->set_build_world(world);
    if (fhe::build_string_op(*c, op, a_cap, b_cap, clear, clear_len) || c->finalize(world)) {
        delete c;
        return 1;
    }
    *out = new fhe_plan{c, true};
    return 0;
}

static int int_plan(const fhe_params_t& params, fhe::Engine* eng, const char* op, uint32_t n_blocks, uint64_t scalar,
                    uint32_t world, fhe_plan** out) {
    fhe::Circuit* c = new fhe::Circuit(params, eng);
    c->set_build_world(world);
    if (fhe::build_integer_op(*c, op, n_blocks, scalar) || c->finalize(world)) {
        delete c;
        return 1;
    }
    *out = new fhe_plan{c, true};
    return 0;
}

int fhe_int_plan_create(fhe_engine* eng, const char* op, uint32_t n_blocks, uint64_t scalar, uint32_t world, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(op);
    return int_plan(eng->impl->p, eng->impl, op, n_blocks, scalar, world, out);
    API_END
}

int fhe_int_plan_create_offline(const fhe_params_t* params, const char* op, uint32_t n_blocks, uint64_t scalar,
                                uint32_t world, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(params); CHECK_PTR(op);
    return int_plan(*params, nullptr, op, n_blocks, scalar, world, out);
    API_END
}

int fhe_str_plan_create_offline(const fhe_params_t* params, const char* op, uint32_t a_cap, uint32_t b_cap,
                                const uint8_t* clear, uint32_t clear_len, uint32_t world, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(params); CHECK_PTR(op);
    return str_plan(*params, nullptr, op, a_cap, b_cap, clear, clear_len, world, out);
    API_END
}

int fhe_plan_lut_count(const fhe_plan* p, uint32_t* count) {
    API_BEGIN
    CHECK_PTR(p); CHECK_PTR(count);
    *count = p->c->n_luts();
    return 0;
    API_END
}

int fhe_plan_export_lut(const fhe_plan* p, uint32_t lut, uint64_t* accumulator) {
    API_BEGIN
    CHECK_PTR(p); CHECK_PTR(accumulator);
    if (lut >= p->c->n_luts()) return fail("bad plan LUT id");
    const auto& acc = p->c->lut_accumulator(lut);
    std::copy(acc.begin(), acc.end(), accumulator);
    return 0;
    API_END
}

int fhe_str_plan_create(fhe_engine* eng, const char* op, uint32_t a_cap, uint32_t b_cap,
                        const uint8_t* clear, uint32_t clear_len, uint32_t world, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(op);
    return str_plan(eng->impl->p, eng->impl, op, a_cap, b_cap, clear, clear_len, world, out);
    API_END
}

int fhe_plan_info(const fhe_plan* p, uint32_t info[6]) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(info);
    info[0] = p->c->n_inputs(); info[1] = p->c->n_outputs(); info[2] = p->c->n_levels();
    info[3] = p->c->n_pbs(); info[4] = p->c->pool_slots(); info[5] = p->c->world();
    return 0;
    API_END
}

static const fhe::Circuit::Level* plan_level(const fhe_plan* p, uint32_t level) {
    if (level < p->c->n_levels()) return &p->c->level(level);
    if (level == p->c->n_levels()) return &p->c->out_level();
    return nullptr;
}

int fhe_plan_level_info(const fhe_plan* p, uint32_t level, uint32_t info[8]) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(info);
    const auto* lv = plan_level(p, level);
    if (!lv) return fail("bad level");
    info[0] = (uint32_t)lv->off.size() - 1; info[1] = lv->local_base; info[2] = lv->local_size;
    info[3] = lv->e_max; info[4] = lv->recv_base; info[5] = (uint32_t)lv->src.size();
    info[6] = info[7] = 0;
    return 0;
    API_END
}

int fhe_plan_level_rank_info(const fhe_plan* p, uint32_t level, uint32_t rank, uint32_t info[3]) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(info);
    if (level >= p->c->n_levels()) return fail("bad level");
    if (rank >= p->c->world()) return fail("bad rank");
    const auto& lv = p->c->level(level);
    info[0] = lv.rank_off[rank]; info[1] = lv.rank_off[rank + 1]; info[2] = lv.n_export[rank];
    return 0;
    API_END
}

int fhe_plan_noise_info(const fhe_plan* p, double info[4]) {
    API_BEGIN
    CHECK_PTR(p); CHECK_PTR(info);
    const fhe::NoiseModel m = fhe::noise_model(p->c->params());
    info[0] = p->c->max_pbs_input_noise();
    info[1] = p->c->noise_budget();
    info[2] = m.log2_pfail(p->c->max_pbs_input_noise());
    info[3] = (double)p->c->gathered_lwes();
    return 0;
    API_END
}

int fhe_noise_model(const fhe_params_t* params, double out[6]) {
    API_BEGIN
    CHECK_PTR(params); CHECK_PTR(out);
    const fhe::NoiseModel m = fhe::noise_model(*params);
    out[0] = m.v_pbs; out[1] = m.v_ks; out[2] = m.v_ms; out[3] = m.half_box;
    out[4] = fhe::default_noise_budget(*params); out[5] = m.log2_pfail(out[4]);
    return 0;
    API_END
}

int fhe_host_alloc(size_t bytes, void** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    if (bytes == 0) return 0;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { *out = nullptr; return fhe::fail("fhe_host_alloc: hipHostMalloc failed"); }
    return 0;
    API_END
}

int fhe_host_free(void* ptr) {
    API_BEGIN
    if (ptr && hipHostFree(ptr) != hipSuccess) return fhe::fail("fhe_host_free: not a buffer of fhe_host_alloc");
    return 0;
    API_END
}

int fhe_params_supported(const fhe_params_t* params) {
    API_BEGIN
    CHECK_PTR(params);
    return fhe::params_supported(*params);
    API_END
}

int fhe_noise_model_is_calibrated(const fhe_params_t* params) {
    return params && fhe::noise_model_is_calibrated(*params) ? 1 : 0;
}

int fhe_plan_set_noise_budget(fhe_plan* p, double budget) {
    API_BEGIN
    PLAN_BUILDING(p);
    p->c->set_noise_budget(budget);
    return 0;
    API_END
}

int fhe_plan_export_level(const fhe_plan* p, uint32_t level, uint32_t* off, uint32_t* src,
                          int32_t* coeff, uint64_t* cst, uint32_t* lut) {
    API_BEGIN
    PLAN_READY(p);
    const auto* lv = plan_level(p, level);
    if (!lv) return fail("bad level");
    if (off) std::copy(lv->off.begin(), lv->off.end(), off);
    if (src) std::copy(lv->src.begin(), lv->src.end(), src);
    if (coeff) std::copy(lv->coeff.begin(), lv->coeff.end(), coeff);
    if (cst) std::copy(lv->cst.begin(), lv->cst.end(), cst);
    if (lut) std::copy(lv->lut.begin(), lv->lut.end(), lut);
    return 0;
    API_END
}

int fhe_plan_run(fhe_plan* p, const uint64_t* inputs, uint64_t* outputs) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(outputs);
    if (p->c->n_inputs()) CHECK_PTR(inputs);
    return p->c->run_host(inputs, outputs);
    API_END
}

int fhe_plan_run_batch(fhe_plan* p, uint32_t instances, const uint64_t* inputs, uint64_t* outputs) {
    API_BEGIN
    PLAN_READY(p);
    if (instances == 0) return 0;
    CHECK_PTR(outputs);
    if (p->c->n_inputs()) CHECK_PTR(inputs);
    return p->c->run_batch_host(inputs, p->c->n_inputs(), nullptr, outputs, instances);
    API_END
}

int fhe_plan_run_batch_dev(fhe_plan* p, uint32_t instances, const uint64_t* d_inputs, uint64_t* d_outputs) {
    API_BEGIN
    PLAN_READY(p);
    if (instances == 0) return 0;
    CHECK_PTR(d_outputs);
    if (p->c->n_inputs()) CHECK_PTR(d_inputs);
    return p->c->run_batch_dev(d_inputs, d_outputs, instances);
    API_END
}

int fhe_plan_run_level_rank_dev(fhe_plan* p, uint64_t* d_pool, uint32_t level, uint32_t rank) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(d_pool);
    return p->c->run_level_rank(d_pool, level, rank);
    API_END
}

int fhe_plan_gather_outputs_dev(fhe_plan* p, const uint64_t* d_pool, uint64_t* d_out) {
    API_BEGIN
    PLAN_READY(p); CHECK_PTR(d_pool); CHECK_PTR(d_out);
    return p->c->gather_outputs(d_pool, d_out);
    API_END
}

// plan cache of the one-call string operations, most recently used first (at most STR_PLAN_CACHE entries)
static int cached_str_plan(fhe_engine* eng, const std::string& op, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len,
                           fhe_plan** out) {
    constexpr size_t STR_PLAN_CACHE = 8;
    std::string key = op + "|" + std::to_string(a_cap) + "|" + std::to_string(b_cap) + "|";
    if (clear) key.append(reinterpret_cast<const char*>(clear), clear_len);
    fhe_plan* plan = nullptr;
    auto& cache = eng->str_plans;
    for (size_t i = 0; i < cache.size(); i++)
        if (cache[i].first == key) {
            plan = cache[i].second;
            std::rotate(cache.begin(), cache.begin() + i, cache.begin() + i + 1);
            break;
        }
    if (!plan) {
        if (fhe_str_plan_create(eng, op.c_str(), a_cap, b_cap, clear, clear_len, 1, &plan)) return 1;
        cache.insert(cache.begin(), {key, plan});
        if (cache.size() > STR_PLAN_CACHE) {
            fhe_plan_destroy(cache.back().second);
            cache.pop_back();
        }
    }
    *out = plan;
    return 0;
}

// One run of a cached FheString plan on host buffers, by plan name (include/fhestr.h): every one-call string entry point
// below is a shorthand that ends here.  operands: up to three encrypted strings of caps[i] characters, the plan's first
// inputs; n_digits: the digits of an encrypted count, the plan's last inputs (NULL: the plan takes none).
int fhe_str_op(fhe_engine* eng, const char* name, const uint64_t* const* operands, const uint32_t* caps, uint32_t n_operands,
               const uint64_t* n_digits, const uint8_t* clear, uint32_t clear_len, uint64_t* out, uint32_t* n_outputs) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(name); CHECK_PTR(operands); CHECK_PTR(caps);
    if (n_operands < 1 || n_operands > 3) return fail("fhe_str_op: one to three encrypted string operands");
    const std::string op(name);
    const bool query = !out && n_outputs;
    if (!query) CHECK_PTR(out);
    uint32_t b_cap = 0;
    for (uint32_t i = 0; i < n_operands; i++) {
        if (!query) CHECK_PTR(operands[i]);
        if (i) b_cap += caps[i];
    }
    fhe_plan* plan = nullptr;
    if (cached_str_plan(eng, op, caps[0], b_cap, clear, clear_len, &plan)) return 1;
    if (n_outputs) *n_outputs = plan->c->n_outputs();
    if (query) return 0;
    const uint32_t bpc = fhe::opname::blocks_per_char(plan->c->msg_modulus());
    const uint64_t* parts[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t counts[4] = {0, 0, 0, 0}, placed = 0;
    for (uint32_t i = 0; i < n_operands; i++) {
        parts[i] = operands[i];
        placed += counts[i] = caps[i] * bpc;
    }
    if (n_digits) {
        if (placed >= plan->c->n_inputs()) return fail(op + ": the plan has no input left for the count's digits");
        parts[n_operands] = n_digits;
        counts[n_operands] = plan->c->n_inputs() - placed;
    }
    return plan->c->run_host_parts(parts, counts, n_operands + (n_digits ? 1 : 0), out);
    API_END
}

// the clear operand of the replace forms: from || to
static std::vector<uint8_t> join(const uint8_t* from, uint32_t from_len, const uint8_t* to, uint32_t to_len) {
    std::vector<uint8_t> joined(from, from + from_len);
    joined.insert(joined.end(), to, to + to_len);
    return joined;
}

// the shorthands on one string and at most one encrypted operand
static int str_op_ab(fhe_engine* eng, const char* op, const uint64_t* a, uint32_t a_cap, const uint64_t* b,
                     uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, uint64_t* out) {
    if (!a) return fail("null pointer: a");
    const uint64_t* operands[2] = {a, b};
    const uint32_t caps[2] = {a_cap, b_cap};
    return fhe_str_op(eng, op, operands, caps, b ? 2 : 1, nullptr, clear, clear_len, out, nullptr);
}

// `count` strings against ONE second operand in one pass (Circuit::run_batch_host): level l of all rows is one launch.
int fhe_str_op_many(fhe_engine* eng, const char* op, const uint64_t* rows, uint32_t a_cap, uint32_t count, const uint64_t* b, uint32_t b_cap,
                    const uint8_t* clear, uint32_t clear_len, uint64_t* out, uint32_t* n_outputs) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(op);
    fhe_plan* plan = nullptr;
    if (cached_str_plan(eng, op, a_cap, b_cap, clear, clear_len, &plan)) return 1;
    if (n_outputs) *n_outputs = plan->c->n_outputs();
    if (!out && n_outputs) return 0;                    // query: how many output ciphertexts per row
    CHECK_PTR(rows); CHECK_PTR(out);
    if (b_cap && !b) return fail("null pointer: b");
    if (a_cap + b_cap == 0) return fail("fhe_str_op_many: empty operands");
    const uint32_t bpc = fhe::opname::blocks_per_char(plan->c->msg_modulus());
    // what the rows do not bring is shared: the second operand, then the digits of an encrypted count
    const bool shares = plan->c->n_inputs() > a_cap * bpc;
    if (shares && !b) return fail("null pointer: b (the shared operand: the pattern, then the digits of an encrypted count)");
    return plan->c->run_batch_host(rows, a_cap * bpc, shares ? b : nullptr, out, count);
    API_END
}

#define STR_BINARY(name)                                                                              \
    int fhe_str_##name(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* b,         \
                       uint32_t b_cap, uint64_t* out) {                                               \
        if (!b) return fail("null pointer: b");                                                       \
        return str_op_ab(eng, #name, a, a_cap, b, b_cap, nullptr, 0, out);                               \
    }                                                                                                 \
    int fhe_str_##name##_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* pat, \
                               uint32_t pat_len, uint64_t* out) {                                     \
        return str_op_ab(eng, #name "_clear", a, a_cap, nullptr, 0, pat, pat_len, out);                  \
    }
STR_BINARY(eq)
STR_BINARY(ne)
STR_BINARY(starts_with)
STR_BINARY(ends_with)
STR_BINARY(contains)
STR_BINARY(find)
STR_BINARY(rfind)
STR_BINARY(eq_ignore_case)
STR_BINARY(lt)
STR_BINARY(le)
STR_BINARY(gt)
STR_BINARY(ge)
STR_BINARY(concat)

/* a clear regular expression (the pattern text /.../ of regex.h): out = one 0/1 block */
int fhe_str_matches_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* regex, uint32_t regex_len, uint64_t* out) {
    if (regex_len && !regex) return fail("null pointer: regex");
    return str_op_ab(eng, "matches_clear", a, a_cap, nullptr, 0, regex, regex_len, out);
}
int fhe_regex_check(const uint8_t* regex, uint32_t len, uint32_t* n_positions, uint32_t* max_len) {
    API_BEGIN
    if (len && !regex) return fail("null pointer: regex");
    fhe::regex::Automaton g;
    std::string why;
    if (fhe::regex::compile(regex, len, g, why)) return fail("regex: " + why);
    if (n_positions) *n_positions = g.positions();
    if (max_len) *max_len = g.max_len;
    return 0;
    API_END
}

/* encrypted (zero padded) pattern: out = 1 + a_cap * blocks LWEs, stripped bit first */
int fhe_str_strip_prefix(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* pat, uint32_t pat_cap, uint64_t* out) {
    if (!pat) return fail("null pointer: pat");
    return str_op_ab(eng, "strip_prefix", a, a_cap, pat, pat_cap, nullptr, 0, out);
}
int fhe_str_strip_suffix(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* pat, uint32_t pat_cap, uint64_t* out) {
    if (!pat) return fail("null pointer: pat");
    return str_op_ab(eng, "strip_suffix", a, a_cap, pat, pat_cap, nullptr, 0, out);
}
int fhe_str_replace_general(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* from, uint32_t from_cap,
                            const uint64_t* to, uint32_t to_cap, uint32_t out_cap, uint64_t* out) {
    if (!a) return fail("null pointer: a");
    if (!from || from_cap == 0) return fail("replace: `from` needs a capacity of at least one character");
    if (to_cap && !to) return fail("null pointer: to");
    const std::string op = "replace:" + std::to_string(from_cap) + ":" + std::to_string(out_cap);
    const uint64_t* operands[3] = {a, from, to};
    const uint32_t caps[3] = {a_cap, from_cap, to_cap};
    return fhe_str_op(eng, op.c_str(), operands, caps, to_cap ? 3 : 2, nullptr, nullptr, 0, out, nullptr);
}
int fhe_str_replace_clear_general(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* from, uint32_t from_len,
                                  const uint8_t* to, uint32_t to_len, uint32_t out_cap, uint64_t* out) {
    if ((from_len && !from) || (to_len && !to)) return fail("null pointer: from / to");
    const std::vector<uint8_t> both = join(from, from_len, to, to_len);
    const std::string op = "replace_clear:" + std::to_string(from_len) + ":" + std::to_string(out_cap);
    return str_op_ab(eng, op.c_str(), a, a_cap, nullptr, 0, both.data(), (uint32_t)both.size(), out);
}

int fhe_str_replacen(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* from, uint32_t from_cap,
                     const uint64_t* to, uint32_t to_cap, uint32_t n, uint32_t out_cap, uint64_t* out) {
    if (!a) return fail("null pointer: a");
    if (!from || from_cap == 0) return fail("replacen: `from` needs a capacity of at least one character");
    if (to_cap && !to) return fail("null pointer: to");
    const std::string op = "replacen:" + std::to_string(n) + ":" + std::to_string(from_cap) + ":" + std::to_string(out_cap);
    const uint64_t* operands[3] = {a, from, to};
    const uint32_t caps[3] = {a_cap, from_cap, to_cap};
    return fhe_str_op(eng, op.c_str(), operands, caps, to_cap ? 3 : 2, nullptr, nullptr, 0, out, nullptr);
}
int fhe_str_replacen_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* from, uint32_t from_len,
                           const uint8_t* to, uint32_t to_len, uint32_t n, uint32_t out_cap, uint64_t* out) {
    if ((from_len && !from) || (to_len && !to)) return fail("null pointer: from / to");
    const std::vector<uint8_t> both = join(from, from_len, to, to_len);
    const std::string op = "replacen_clear:" + std::to_string(n) + ":" + std::to_string(from_len) + ":" + std::to_string(out_cap);
    return str_op_ab(eng, op.c_str(), a, a_cap, nullptr, 0, both.data(), (uint32_t)both.size(), out);
}

// the split family: one plan name per (operation, clear / encrypted pattern, max_parts, part capacity)
int fhe_str_split(fhe_engine* eng, const char* op, const uint64_t* a, uint32_t a_cap, const uint64_t* pat, uint32_t pat_cap,
                  const uint8_t* clear, uint32_t clear_len, uint32_t max_parts, uint32_t part_cap, uint64_t* out,
                  uint32_t* n_outputs) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(op);
    const std::string base(op);
    const fhe::opname::Row* row = fhe::opname::find_row(base);          // a split row; the encrypted-count ones: fhe_str_splitn_encn
    if (!row || row->family != fhe::opname::SPLIT || row->split.enc_count) return fail("fhe_str_split: unknown operation: " + base);
    if (pat && (clear || clear_len)) return fail("fhe_str_split: give an encrypted pattern or a clear one, not both");
    if (pat && pat_cap == 0) return fail("fhe_str_split: the encrypted pattern needs a capacity of at least one character");
    const bool takes_pattern = !row->unary();
    if (!takes_pattern && (pat || clear || clear_len)) return fail("split_ascii_whitespace takes no pattern");
    if (takes_pattern && !pat && !clear && clear_len) return fail("null clear pattern");
    const bool is_clear = takes_pattern && !pat;        // (an empty clear pattern is refused by the builder)
    std::string name = base + (is_clear ? "_clear" : "");
    if (!row->split.once) name += ":" + std::to_string(max_parts);
    if (part_cap) name += ":" + std::to_string(part_cap);
    if (out || !n_outputs) CHECK_PTR(a);                // (not a query)
    const uint64_t* operands[2] = {a, pat};
    const uint32_t caps[2] = {a_cap, pat ? pat_cap : 0};
    return fhe_str_op(eng, name.c_str(), operands, caps, pat ? 2 : 1, nullptr, is_clear ? clear : nullptr, is_clear ? clear_len : 0, out, n_outputs);
    API_END
}

// ---- encrypted counts: the D digits of n are the plan's last inputs (include/fhestr.h) ----
int fhe_str_repeat(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* n_digits, uint32_t max_count, uint64_t* out) {
    if (max_count == 0 || max_count > 255) return fail("repeat: max_count must be in 1..255");
    CHECK_PTR(n_digits);
    const uint64_t* operands[1] = {a};
    return fhe_str_op(eng, ("repeat:" + std::to_string(max_count)).c_str(), operands, &a_cap, 1, n_digits, nullptr, 0, out, nullptr);
}
int fhe_str_replacen_encn(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* from, uint32_t from_cap,
                          const uint64_t* to, uint32_t to_cap, const uint64_t* n_digits, uint32_t n_max, uint32_t out_cap, uint64_t* out) {
    if (!from || from_cap == 0) return fail("replacen: `from` needs a capacity of at least one character");
    if (to_cap && !to) return fail("null pointer: to");
    CHECK_PTR(n_digits);
    const std::string op = "replacen_encn:" + std::to_string(n_max) + ":" + std::to_string(from_cap) + ":" + std::to_string(out_cap);
    const uint64_t* operands[3] = {a, from, to};
    const uint32_t caps[3] = {a_cap, from_cap, to_cap};
    return fhe_str_op(eng, op.c_str(), operands, caps, to_cap ? 3 : 2, n_digits, nullptr, 0, out, nullptr);
}
int fhe_str_replacen_encn_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* from, uint32_t from_len,
                                const uint8_t* to, uint32_t to_len, const uint64_t* n_digits, uint32_t n_max, uint32_t out_cap,
                                uint64_t* out) {
    if ((from_len && !from) || (to_len && !to)) return fail("null pointer: from / to");
    CHECK_PTR(n_digits);
    const std::vector<uint8_t> both = join(from, from_len, to, to_len);
    const std::string op = "replacen_encn_clear:" + std::to_string(n_max) + ":" + std::to_string(from_len) + ":" + std::to_string(out_cap);
    const uint64_t* operands[1] = {a};
    return fhe_str_op(eng, op.c_str(), operands, &a_cap, 1, n_digits, both.data(), (uint32_t)both.size(), out, nullptr);
}
int fhe_str_splitn_encn(fhe_engine* eng, const char* op, const uint64_t* a, uint32_t a_cap, const uint64_t* pat, uint32_t pat_cap,
                        const uint8_t* clear, uint32_t clear_len, const uint64_t* n_digits, uint32_t max_parts, uint32_t part_cap,
                        uint64_t* out, uint32_t* n_outputs) {
    if (!op) return fail("null pointer: op");
    const std::string base(op);
    const fhe::opname::Row* row = fhe::opname::find_row(base + "_encn");
    if (!row || !row->split.enc_count) return fail("fhe_str_splitn_encn: op must be \"splitn\" or \"rsplitn\", got: " + base);
    if (pat && (clear || clear_len)) return fail("fhe_str_splitn_encn: give an encrypted pattern or a clear one, not both");
    if (pat && pat_cap == 0) return fail("fhe_str_splitn_encn: the encrypted pattern needs a capacity of at least one character");
    if (!pat && !clear && clear_len) return fail("null clear pattern");
    if (out || !n_outputs) CHECK_PTR(n_digits);         // (not a query)
    std::string name = base + "_encn" + (pat ? "" : "_clear") + ":" + std::to_string(max_parts);
    if (part_cap) name += ":" + std::to_string(part_cap);
    const uint64_t* operands[2] = {a, pat};
    const uint32_t caps[2] = {a_cap, pat ? pat_cap : 0};
    return fhe_str_op(eng, name.c_str(), operands, caps, pat ? 2 : 1, n_digits, pat ? nullptr : clear, pat ? 0 : clear_len, out, n_outputs);
}
// the slice family: one plan name per (operation, clear / encrypted position, clear / encrypted t, output capacity)
int fhe_str_slice(fhe_engine* eng, const char* op, const uint64_t* a, uint32_t a_cap, const uint64_t* t, uint32_t t_cap,
                  const uint8_t* clear, uint32_t clear_len, const uint64_t* n_digits, uint32_t n_or_n_max, uint32_t out_cap,
                  uint64_t* out, uint32_t* n_outputs) {
    if (!op) return fail("null pointer: op");
    const std::string base(op);
    const fhe::opname::Row* row = fhe::opname::find_row(base);
    if (!row || row->family != fhe::opname::SLICE || row->split.enc_count)
        return fail("fhe_str_slice: op must be \"take\", \"skip\", \"split_at\", \"char_at\" or \"insert\", got: " + base);
    const bool inserts = row->how == fhe::opname::INSERT;
    if (!inserts && (t || clear || clear_len)) return fail("fhe_str_slice: only insert takes a string to insert");
    if (t && (clear || clear_len)) return fail("fhe_str_slice: give an encrypted string to insert or a clear one, not both");
    if (t && t_cap == 0) return fail("fhe_str_slice: the encrypted string to insert needs a capacity of at least one character");
    if (!t && !clear && clear_len) return fail("null clear pattern");
    const bool is_clear = inserts && !t;
    std::string name = base + (n_digits ? "_encn" : "") + (is_clear ? "_clear" : "") + ":" + std::to_string(n_or_n_max);
    if (out_cap) name += ":" + std::to_string(out_cap);
    if (out || !n_outputs) {                            // (not a query)
        if (!a) return fail("null pointer: a");
    }
    const uint64_t* operands[2] = {a, t};
    const uint32_t caps[2] = {a_cap, t ? t_cap : 0};
    return fhe_str_op(eng, name.c_str(), operands, caps, t ? 2 : 1, n_digits, is_clear ? clear : nullptr, is_clear ? clear_len : 0, out, n_outputs);
}

// the names that combine results: operands of any kind, in the plan's input order, checked against the name's shape
int fhe_str_combine(fhe_engine* eng, const char* name, const uint64_t* const* operands, const uint32_t* n_blocks, uint32_t n_operands,
                    const uint8_t* clear, uint32_t clear_len, uint64_t* out, uint32_t* n_outputs) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(name);
    if (n_operands) { CHECK_PTR(operands); CHECK_PTR(n_blocks); }
    const std::string op(name);
    const fhe::opname::Name n = fhe::opname::parse(op);
    if (n.status != fhe::opname::OK || !n.combines())
        return fail("fhe_str_combine: not a name that combines results (and or xor not select select_count count_...): " + op);
    const bool query = !out && n_outputs;
    if (!query) CHECK_PTR(out);
    const uint32_t msg_mod = eng->impl->p.msg_mod, bpc = fhe::opname::blocks_per_char(msg_mod);
    if (bpc == 0) return fail("string ops need msg_mod = 2^b with b | 8 and carry_mod >= msg_mod");
    std::vector<uint32_t> caps;
    if (n.is(fhe::opname::SELECT) && n.row->how == fhe::opname::OF_STRINGS)
        for (uint32_t i = 0; i < (n.clear ? 1u : 2u) && i < n_operands; i++) {
            if (n_blocks[i] == 0 || n_blocks[i] % bpc)
                return fail(op + ": operand " + std::to_string(i) + " is a string: " + std::to_string(n_blocks[i]) + " blocks are no whole characters of " +
                            std::to_string(bpc) + " blocks");
            caps.push_back(n_blocks[i] / bpc);
        }
    const uint32_t a_cap = caps.empty() ? 0 : caps[0], b_cap = caps.size() > 1 ? caps[1] : 0;
    fhe::program::OpLayout lay;
    std::string why;
    if (fhe::program::op_layout(op, msg_mod, caps.data(), (uint32_t)caps.size(), clear, clear_len, lay, why)) return fail(why);
    if (lay.known) {
        static const char* const kinds[] = {"string", "bit", "count"};
        if (n_operands != lay.operands.size())
            return fail(op + ": takes " + std::to_string(lay.operands.size()) + " operand(s), got " + std::to_string(n_operands));
        for (uint32_t i = 0; i < n_operands; i++) {
            if (!query) CHECK_PTR(operands[i]);
            if (n_blocks[i] != lay.operands[i].blocks)
                return fail(op + ": operand " + std::to_string(i) + " has " + std::to_string(n_blocks[i]) + " blocks, the name takes a " +
                            kinds[lay.operands[i].kind] + " of " + std::to_string(lay.operands[i].blocks));
        }
    }
    fhe_plan* plan = nullptr;               // (a name the shape refuses: the builder says why)
    if (cached_str_plan(eng, op, a_cap, b_cap, clear, clear_len, &plan)) return 1;
    if (!lay.known) return fail("internal: " + op + " builds and has no layout");
    if (n_outputs) *n_outputs = plan->c->n_outputs();
    if (query) return 0;
    return plan->c->run_host_parts(operands, n_blocks, n_operands, out);
    API_END
}

int fhe_str_repeat_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint32_t count, uint64_t* out) {
    if (count == 0 || count > 255) return fail("repeat: count must be in 1..255");
    const uint8_t c = (uint8_t)count;
    return str_op_ab(eng, "repeat_clear", a, a_cap, nullptr, 0, &c, 1, out);
}

int fhe_str_replace(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint64_t* from_to,
                    uint32_t pat_cap, uint64_t* out) {
    if (!from_to) return fail("null pointer: from_to");
    return str_op_ab(eng, "replace", a, a_cap, from_to, 2 * pat_cap, nullptr, 0, out);
}
int fhe_str_replace_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* from,
                          const uint8_t* to, uint32_t pat_len, uint64_t* out) {
    if (pat_len && (!from || !to)) return fail("null pointer: from / to");
    const std::vector<uint8_t> both = join(from, pat_len, to, pat_len);
    return str_op_ab(eng, "replace_clear", a, a_cap, nullptr, 0, both.data(), 2 * pat_len, out);
}
int fhe_str_trim_start(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "trim_start", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_trim_end(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "trim_end", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_strip(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "strip", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_len(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "len", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_is_empty(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "is_empty", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_strip_prefix_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* pat,
                               uint32_t pat_len, uint64_t* out) {
    return str_op_ab(eng, "strip_prefix_clear", a, a_cap, nullptr, 0, pat, pat_len, out);
}
int fhe_str_strip_suffix_clear(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, const uint8_t* pat,
                               uint32_t pat_len, uint64_t* out) {
    return str_op_ab(eng, "strip_suffix_clear", a, a_cap, nullptr, 0, pat, pat_len, out);
}
int fhe_str_to_upper(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "to_upper", a, a_cap, nullptr, 0, nullptr, 0, out);
}
int fhe_str_to_lower(fhe_engine* eng, const uint64_t* a, uint32_t a_cap, uint64_t* out) {
    return str_op_ab(eng, "to_lower", a, a_cap, nullptr, 0, nullptr, 0, out);
}

// ---- string programs: several FheString operations in one plan (str_program.h) ----
}  // extern "C"

namespace {
// the program builder's view of a Circuit
struct CircuitBackend final : fhe::program::Backend {
    fhe::Circuit* c = nullptr;
    uint32_t msg_modulus() const override { return c->msg_modulus(); }
    uint32_t input(uint64_t degree) override { return c->input(degree); }
    uint32_t trivial(int64_t value) override { return c->trivial(value); }
    void set_dedupe(bool on) override { c->set_dedupe(on); }
    void bind_inputs(const std::vector<uint32_t>& nodes) override { c->bind_inputs(nodes); }
    std::string end_binding() override {
        c->end_binding();
        return c->error();
    }
    uint32_t n_outputs() const override { return c->n_outputs(); }
    std::vector<uint32_t> take_outputs(uint32_t mark) override { return c->take_outputs(mark); }
    void output(uint32_t node) override { c->output(node); }
    int build_op(const std::string& op, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len,
                 std::string& why) override {
        if (!fhe::build_string_op(*c, op, a_cap, b_cap, clear, clear_len)) return 0;
        why = fhe::g_last_error;
        return 1;
    }
};
}  // namespace

struct fhe_str_program {
    CircuitBackend backend;            // owns the circuit until finish hands it to the plan
    fhe::program::Program prog;
    fhe::Engine* eng;                  // whose lock guards the circuit; null: offline, or finished (nothing left to guard)
    explicit fhe_str_program(fhe::Circuit* c) : prog((backend.c = c, backend)), eng(c->engine()) {}
};

#define LOCK_PROGRAM(p) \
    std::unique_lock<std::recursive_mutex> _program_lock; \
    if ((p)->eng) _program_lock = std::unique_lock<std::recursive_mutex>((p)->eng->mu)

extern "C" {

int fhe_str_program_create(fhe_engine* eng, fhe_str_program** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng);
    *out = new fhe_str_program(new fhe::Circuit(eng->impl->p, eng->impl));
    return 0;
    API_END
}

int fhe_str_program_create_offline(const fhe_params_t* params, fhe_str_program** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(params);
    *out = new fhe_str_program(new fhe::Circuit(*params, nullptr));
    return 0;
    API_END
}

int fhe_str_program_destroy(fhe_str_program* prog) {
    API_BEGIN
    if (!prog) return 0;
    {
        LOCK_PROGRAM(prog);        // the circuit's destructor releases device memory of the engine's GPU
        delete prog->backend.c;
    }
    delete prog;
    return 0;
    API_END
}

int fhe_str_program_set_dedupe(fhe_str_program* prog, int on) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog);
    std::string why;
    return prog->prog.set_dedupe(on != 0, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_input_string(fhe_str_program* prog, uint32_t cap, uint32_t* value) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog); CHECK_PTR(value);
    std::string why;
    return prog->prog.input_string(cap, *value, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_input_count(fhe_str_program* prog, uint32_t n_max, uint32_t* value) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog); CHECK_PTR(value);
    std::string why;
    return prog->prog.input_count(n_max, *value, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_input_bit(fhe_str_program* prog, uint32_t* value) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog); CHECK_PTR(value);
    std::string why;
    return prog->prog.input_bit(*value, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_op(fhe_str_program* prog, const char* op, const uint32_t* operands, uint32_t n_operands, const uint8_t* clear,
                       uint32_t clear_len, uint32_t* results, uint32_t results_cap, uint32_t* n_results) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog); CHECK_PTR(op); CHECK_PTR(n_results);
    std::string why;
    return prog->prog.op(op, operands, n_operands, clear, clear_len, results, results_cap, *n_results, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_value_info(const fhe_str_program* prog, uint32_t value, uint32_t info[4]) {
    API_BEGIN
    CHECK_PTR(prog); CHECK_PTR(info);
    const fhe::program::Value* v;
    std::string why;
    if (prog->prog.value(value, v, why)) return fail(why);
    info[0] = v->kind; info[1] = (uint32_t)v->nodes.size(); info[2] = v->extent; info[3] = v->op_index;
    return 0;
    API_END
}

int fhe_str_program_output(fhe_str_program* prog, uint32_t value) {
    API_BEGIN
    CHECK_PTR(prog); LOCK_PROGRAM(prog);
    std::string why;
    return prog->prog.output(value, why) ? fail(why) : 0;
    API_END
}

int fhe_str_program_finish(fhe_str_program* prog, uint32_t world, fhe_plan** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(prog); LOCK_PROGRAM(prog);
    std::string why;
    if (prog->prog.can_finish(why)) return fail(why);
    if (prog->backend.c->finalize(world)) return 1;
    if (prog->prog.finish(why)) return fail(why);
    *out = new fhe_plan{prog->backend.c, true};
    prog->backend.c = nullptr;      // the plan owns the circuit from here on ...
    prog->eng = nullptr;            // ... and the program, now a table of values, may outlive the engine
    return 0;
    API_END
}

// ---- transciphering (stream_cipher.h, transcipher.h; the device side: transcipher_dev.hip) ----------------------------
static int tc_answer(const char* why) { return why ? fail(why) : 0; }

int fhe_stream_cipher_info(uint32_t cipher, uint32_t info[3]) {
    API_BEGIN
    CHECK_PTR(info);
    info[0] = info[1] = info[2] = 0;
    if (!fhe::stream_cipher_ok(cipher)) return fail("stream cipher: unknown cipher (FHE_STREAM_TRIVIUM or FHE_STREAM_KREYVIUM)");
    info[0] = info[1] = fhe::stream_key_bits(cipher);
    info[2] = fhe::STREAM_WARMUP_STEPS;
    return 0;
    API_END
}

int fhe_stream_cipher_keystream(uint32_t cipher, const uint8_t* key, const uint8_t* iv, uint64_t first_byte, uint8_t* out, size_t n_bytes) {
    API_BEGIN
    CHECK_PTR(key); CHECK_PTR(iv);
    if (n_bytes) CHECK_PTR(out);
    return tc_answer(fhe::stream_keystream(cipher, key, iv, first_byte, out, n_bytes));
    API_END
}

int fhe_transcipher_supported(const fhe_params_t* params, uint32_t cipher) {
    API_BEGIN
    CHECK_PTR(params);
    return tc_answer(fhe::tc_supported(*params, cipher));
    API_END
}

int fhe_transcipher_table(const fhe_params_t* params, uint32_t table, uint64_t* values, uint32_t* n_tables) {
    API_BEGIN
    CHECK_PTR(params); CHECK_PTR(n_tables);
    *n_tables = 0;
    fhe::TcShape sh;
    if (const char* why = fhe::tc_shape(*params, FHE_STREAM_KREYVIUM, 1, &sh)) return fail(why);   // the tables do not depend on the cipher; Kreyvium uses all of them
    *n_tables = fhe::TC_TABLE_G + 2 * sh.bits;
    if (!values) return 0;
    if (table >= *n_tables) return fail("transcipher: table number out of range");
    for (uint32_t v = 0; v < params->msg_mod * params->carry_mod; v++) values[v] = fhe::tc_table_value(table, v);
    return 0;
    API_END
}

size_t fhe_transcipher_ring_len(const fhe_params_t* params, uint32_t streams) {
    return params ? fhe::tc_ring_rows(streams) * ((size_t)params->k * params->N + 1) : 0;
}

int fhe_transcipher_init_host(const fhe_params_t* params, uint32_t cipher, uint32_t streams, const uint64_t* key, const uint8_t* ivs, uint64_t* ring) {
    API_BEGIN
    CHECK_PTR(params); CHECK_PTR(key); CHECK_PTR(ivs); CHECK_PTR(ring);
    fhe::TcShape sh;
    if (const char* why = fhe::tc_shape(*params, cipher, streams, &sh)) return fail(why);
    return tc_answer(fhe::tc_init(sh, key, ivs, ring));
    API_END
}

int fhe_transcipher_gather_host(const fhe_params_t* params, uint32_t cipher, uint32_t streams, int32_t round, uint32_t rows, const uint64_t* ring,
                                const uint64_t* key, const uint8_t* ivs, const uint8_t* data, uint32_t n_bytes, uint32_t m, uint64_t* pbs_in,
                                uint32_t* tables) {
    API_BEGIN
    CHECK_PTR(params); CHECK_PTR(ring); CHECK_PTR(key); CHECK_PTR(ivs); CHECK_PTR(pbs_in); CHECK_PTR(tables);
    fhe::TcShape sh;
    if (const char* why = fhe::tc_shape(*params, cipher, streams, &sh)) return fail(why);
    return tc_answer(fhe::tc_gather(sh, round, rows, ring, key, ivs, rows == fhe::TC_DATA_ROWS ? data : nullptr, n_bytes, m, nullptr, pbs_in, tables));
    API_END
}

int fhe_transcipher_apply_host(const fhe_params_t* params, uint32_t cipher, uint32_t streams, int32_t round, const uint64_t* ring, uint32_t n_bytes,
                               uint32_t m, uint64_t* out) {
    API_BEGIN
    CHECK_PTR(params); CHECK_PTR(ring); CHECK_PTR(out);
    fhe::TcShape sh;
    if (const char* why = fhe::tc_shape(*params, cipher, streams, &sh)) return fail(why);
    if ((uint64_t)8 * m >= n_bytes) return fail("transcipher: round m of a call starts at byte 8 m, past the call's bytes");
    return tc_answer(fhe::tc_apply(sh, round, ring, n_bytes, m, out));
    API_END
}

int fhe_engine_transcipher_init(fhe_engine* eng, uint32_t cipher, uint32_t streams, const uint64_t* key, const uint8_t* ivs, uint64_t* ring) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(key); CHECK_PTR(ivs); CHECK_PTR(ring);
    return eng->impl->transcipher_init_host(cipher, streams, key, ivs, ring);
    API_END
}

int fhe_engine_transcipher_gather(fhe_engine* eng, uint32_t cipher, uint32_t streams, int32_t round, uint32_t rows, const uint64_t* ring,
                                  const uint64_t* key, const uint8_t* ivs, const uint8_t* data, uint32_t n_bytes, uint32_t m, uint64_t* pbs_in,
                                  uint32_t* tables) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(ring); CHECK_PTR(key); CHECK_PTR(ivs); CHECK_PTR(pbs_in); CHECK_PTR(tables);
    return eng->impl->transcipher_gather_host(cipher, streams, round, rows, ring, key, ivs, data, n_bytes, m, pbs_in, tables);
    API_END
}

int fhe_engine_transcipher_apply(fhe_engine* eng, uint32_t cipher, uint32_t streams, int32_t round, const uint64_t* ring, uint32_t n_bytes, uint32_t m,
                                 uint64_t* out) {
    API_BEGIN
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(ring); CHECK_PTR(out);
    return eng->impl->transcipher_apply_host(cipher, streams, round, ring, n_bytes, m, out);
    API_END
}

struct fhe_transcipher {
    fhe_engine* eng;
    fhe::Transcipher* impl;      // owned by eng->impl->transciphers
};

int fhe_transcipher_create(fhe_engine* eng, uint32_t cipher, const uint64_t* key_cts, uint32_t max_streams, fhe_transcipher** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(key_cts);
    fhe::Transcipher* t = nullptr;
    if (fhe::Transcipher::create(*eng->impl, cipher, key_cts, max_streams, &t)) return 1;
    *out = new fhe_transcipher{eng, t};
    return 0;
    API_END
}

int fhe_transcipher_destroy(fhe_transcipher* tc) {
    API_BEGIN
    if (!tc) return 0;
    {
        LOCK_ENGINE(tc->eng);
        fhe::Engine& e = *tc->eng->impl;
        if (e.use() || e.sync_all_streams()) return 1;              // launches in flight still read its buffers
        for (auto it = e.transciphers.begin(); it != e.transciphers.end(); ++it)
            if (it->get() == tc->impl) { e.transciphers.erase(it); break; }
    }
    delete tc;
    return 0;
    API_END
}

int fhe_transcipher_begin(fhe_transcipher* tc, const uint8_t* ivs, uint32_t n_streams) {
    API_BEGIN
    CHECK_PTR(tc); LOCK_ENGINE(tc->eng); CHECK_PTR(ivs);
    return tc->impl->begin(ivs, n_streams);
    API_END
}

int fhe_transcipher_next(fhe_transcipher* tc, const uint8_t* data, uint32_t n_bytes, int refresh, uint64_t* out_host, uint64_t* d_out) {
    API_BEGIN
    CHECK_PTR(tc); LOCK_ENGINE(tc->eng);
    if (n_bytes) CHECK_PTR(data);
    return tc->impl->next(data, n_bytes, refresh, out_host, d_out);
    API_END
}

int fhe_transcipher_info(fhe_transcipher* tc, uint32_t info[8]) {
    API_BEGIN
    CHECK_PTR(tc); LOCK_ENGINE(tc->eng); CHECK_PTR(info);
    tc->impl->info(info);
    return 0;
    API_END
}

int fhe_transcipher_timing(fhe_transcipher* tc, int on, double ms[3], uint32_t* rounds) {
    API_BEGIN
    CHECK_PTR(tc); LOCK_ENGINE(tc->eng);
    tc->impl->timed = on != 0;
    if (ms) for (int i = 0; i < 3; i++) ms[i] = tc->impl->phase_ms[i];
    if (rounds) *rounds = tc->impl->timed_rounds;
    return 0;
    API_END
}

// ---- casting keys (cast.h; the device side: cast_dev.hip; parameters, key generation and the host loop: client.cpp) ----
struct fhe_cast_key {
    fhe_engine* eng;
    fhe::CastKey* impl;          // owned by eng->impl->cast_keys
};

int fhe_cast_key_create(fhe_engine* eng, const fhe_cast_params_t* cp, const uint64_t* key, fhe_cast_key** out) {
    API_BEGIN
    CHECK_PTR(out);
    *out = nullptr;
    CHECK_PTR(eng); LOCK_ENGINE(eng); CHECK_PTR(cp); CHECK_PTR(key);
    fhe::CastKey* k = nullptr;
    if (fhe::CastKey::create(*eng->impl, *cp, key, &k)) return 1;
    *out = new fhe_cast_key{eng, k};
    return 0;
    API_END
}

int fhe_cast_key_destroy(fhe_cast_key* h) {
    API_BEGIN
    if (!h) return 0;
    {
        LOCK_ENGINE(h->eng);
        fhe::Engine& e = *h->eng->impl;
        if (e.use() || e.sync_all_streams()) return 1;              // launches in flight still read its buffers
        for (auto it = e.cast_keys.begin(); it != e.cast_keys.end(); ++it)
            if (it->get() == h->impl) { e.cast_keys.erase(it); break; }
    }
    delete h;
    return 0;
    API_END
}

int fhe_cast_key_info(fhe_cast_key* h, uint32_t info[8]) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng); CHECK_PTR(info);
    h->impl->info(info);
    return 0;
    API_END
}

int fhe_cast_key_set_fused(fhe_cast_key* h, int on) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    h->impl->fused = on != 0;
    return 0;
    API_END
}

int fhe_cast_key_set_input_noise(fhe_cast_key* h, double v_in) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (!(v_in >= 0)) return fail("cast: the declared input noise must be a variance >= 0 in the source's nominal units");
    h->impl->v_in = v_in;
    return 0;
    API_END
}

int fhe_cast_key_set_group(fhe_cast_key* h, uint32_t group) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    return h->impl->set_group(group);
    API_END
}

int fhe_cast_lwes(fhe_cast_key* h, const uint64_t* in, uint32_t count, int mode, uint64_t* out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(in); CHECK_PTR(out); }
    return h->impl->cast_host(in, 0, count, false, mode, out);
    API_END
}

int fhe_cast_lwes_dev(fhe_cast_key* h, const uint64_t* d_in, uint32_t count, int mode, uint64_t* d_out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(d_in); CHECK_PTR(d_out); }
    return h->impl->cast_dev(d_in, 0, count, false, mode, d_out);
    API_END
}

int fhe_cast_packed(fhe_cast_key* h, const uint64_t* glwes, uint32_t first, uint32_t count, int mode, uint64_t* out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(glwes); CHECK_PTR(out); }
    return h->impl->cast_host(glwes, first, count, true, mode, out);
    API_END
}

int fhe_cast_packed_dev(fhe_cast_key* h, const uint64_t* d_glwes, uint32_t first, uint32_t count, int mode, uint64_t* d_out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(d_glwes); CHECK_PTR(d_out); }
    return h->impl->cast_dev(d_glwes, first, count, true, mode, d_out);
    API_END
}

int fhe_cast_narrow(fhe_cast_key* h, const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(narrow); CHECK_PTR(out); }
    return h->impl->cast_narrow_host(narrow, held, bits, first, count, mode, out);
    API_END
}

int fhe_cast_narrow_dev(fhe_cast_key* h, const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* d_out) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng);
    if (count) { CHECK_PTR(d_narrow); CHECK_PTR(d_out); }
    return h->impl->cast_narrow_dev(d_narrow, held, bits, first, count, mode, d_out);
    API_END
}

int fhe_cast_debug_digits(fhe_cast_key* h, const uint64_t* src, uint32_t first, uint32_t count, int packed, int8_t* out, size_t* bytes) {
    API_BEGIN
    CHECK_PTR(h); LOCK_ENGINE(h->eng); CHECK_PTR(bytes);
    if (count && out) CHECK_PTR(src);
    return h->impl->digits_host(src, first, count, packed != 0, out, bytes);
    API_END
}

}  // extern "C"
