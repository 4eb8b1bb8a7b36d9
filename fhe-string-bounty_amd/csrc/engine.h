// engine.h -- internal C++ interface of the engine (the public surface is include/fhestr.h).  Engine's members are defined in
// engine.hip, and in blind_rotate.hip where they need a blind-rotation kernel; Packing's in packing_dev.hip, Transcipher's
// in transcipher_dev.hip, CastKey's in cast_dev.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fhestr.h"
#include "blind_rotate.h"
#include "device_buffer.h"
#include "engine_settings.h"
#include "grid_spans.h"

// bumped whenever a device kernel changes; profiles/r03_counters.json records the revision its
// rocprofv3 counters were taken on and bench.py only attaches them to a matching build
#define FHESTR_KERNEL_REVISION "r04.2"

namespace fhe {

// GGSWs in the bootstrapping key: n (classic PBS) or n/g * 2^g (multi-bit, grouping factor g)
inline uint32_t n_ggsw(const fhe_params_t& p) {
    return p.grouping_factor > 1 ? p.n / p.grouping_factor * (1u << p.grouping_factor) : p.n;
}
// plaintext bit GGSW `sel` of a group encrypts (lwe_multi_bit_bootstrap_key_generation.rs:401-427):
// product over the group's key bits of (s_b if selector bit g-1-b is set else 1 - s_b)
inline uint64_t multi_bit_key_bit(const uint64_t* group_bits, uint32_t g, uint32_t sel) {
    uint64_t prod = 1;
    for (uint32_t b = 0; b < g; b++) prod *= group_bits[b] ^ (((sel >> (g - 1 - b)) & 1) ^ 1);
    return prod;
}

void aes128_round_keys(const uint8_t key[16], uint8_t rk[11][16]);   // seeded_keys.cpp
const uint8_t* aes_sbox();

extern thread_local std::string g_last_error;
// The error of a HIP call, or of a DeviceBuffer operation, under the name of the function that met it.
inline int under(const char* who, hipError_t e) { return e == hipSuccess ? 0 : fail(std::string(who) + ": " + hipGetErrorString(e)); }
inline int under(const char* who, int rc) { return rc ? fail(std::string(who) + ": " + g_last_error) : 0; }

// fill_accumulator: shortint/engine/mod.rs:72-128 (host side, no device needed)
uint64_t fill_accumulator(const fhe_params_t& p, const uint64_t* table, std::vector<uint64_t>& acc);
// the same from torus values per box (tables whose entries are not multiples of delta: Circuit::pbs_full_box)
void fill_accumulator_torus(const fhe_params_t& p, const uint64_t* box_values, std::vector<uint64_t>& acc);

// ---- the ks_pbs throughput modes (Engine::ks_pbs_dev): their streams, events, buffers and hazard records -----------------
struct ByteRange { const char* lo; const char* hi; };
inline bool overlap(const ByteRange& a, const ByteRange& b) { return a.lo < b.hi && b.lo < a.hi; }

// One stream a pipelined call can run on, with what its calls need.  Lane 0 runs on the engine's current stream, which it
// does not own (`stream` stays null: Pipeline::stream_of); lanes 1 .. 3 own theirs.  Lane 0's buffers are also those of every
// serial call; lane 1's small buffer is the second one of mode 1 and of pbs_ks_host.
struct PipeLane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;          // behind the lane's latest mode-2 call
    DeviceBuffer<uint64_t> small;       // small ciphertexts: the keyswitch's output, the blind rotation's input
    DeviceBuffer<int8_t> digits;        // A fragments: signed decomposition digits of the batch being keyswitched
    // byte ranges every mode-2 call of the current run read / wrote on this lane (a later call on ANOTHER lane that touches one
    // of them waits for this lane's latest `done`: stream order then covers all of its earlier calls -- ADVICE r3)
    std::vector<ByteRange> ins, outs;
    // must a call on another lane that reads `in` and writes `out` come after this lane's calls?
    bool blocks(const ByteRange& in, const ByteRange& out) const {
        for (const auto& w : outs)
            if (overlap(in, w) || overlap(out, w)) return true;
        for (const auto& r : ins)
            if (overlap(out, r)) return true;
        return false;
    }
    void remember(const ByteRange& in, const ByteRange& out) { add(ins, in); add(outs, out); }
    static void add(std::vector<ByteRange>& rs, const ByteRange& a) {
        for (auto& r : rs)
            if (r.lo == a.lo && r.hi == a.hi) return;
        if (rs.size() < 32) { rs.push_back(a); return; }
        rs[0].lo = std::min(rs[0].lo, a.lo);          // many distinct buffers: fold into one conservative range
        rs[0].hi = std::max(rs[0].hi, a.hi);
    }
};

struct Pipeline {
    static constexpr int MAX_LANES = 4;
    PipeLane lane[MAX_LANES];
    int ready = 0;                      // lanes ensure() has set up
    int width = 2;                      // lanes the calls of mode 2 rotate over (EngineSettings::overlap_width)
    uint64_t calls = 0;                 // pipelined calls of the current run
    hipEvent_t input_ready = nullptr;   // caller's event the next pipelined keyswitch waits for (one shot)
    // mode 1 hands its two small buffers between the keyswitch stream and the engine's: keyswitch done [slot], blind rotation done [slot]
    hipEvent_t ks_done[2] = {nullptr, nullptr}, rot_done[2] = {nullptr, nullptr};
    ByteRange prev_out[2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // mode 1: what the last call on each buffer wrote
    hipEvent_t run_start = nullptr;     // what the engine's stream held before the run's first call

    template <class F> void each_event(F f) {      // the nine events: they are created together, with the first lanes
        for (auto& l : lane) f(l.done);
        for (int s = 0; s < 2; s++) { f(ks_done[s]); f(rot_done[s]); }
        f(run_start);
    }
    int ensure(int n);                  // lanes 0 .. n-1 exist; what is missing is created whole or not at all, so a failed call can be repeated
    hipStream_t stream_of(int q, hipStream_t engine) const { return q ? lane[q].stream : engine; }
    int wait_others();                  // on the host, for every lane but the engine's
    int wait_all(hipStream_t engine);   // and for the engine's
    void end_run();                     // every lane is idle, or will only be used behind the engine's stream: the next pipelined call starts a new run
    void destroy(int keep = 0);         // after the waits: the streams of lanes keep .. 3 and, with keep = 0, the events
    ~Pipeline() { destroy(); }
};
static_assert(EngineSettings::OVERLAP_MAX == Pipeline::MAX_LANES, "every width the settings accept has its lane");

// The packed-ciphertext family (members in packing_dev.hip): the packing keyswitch (packing_ks_kernels.hip.h), the packed
// inputs (glwe_extract_kernels.hip.h) and the narrow packed results (glwe_narrow.h, glwe_narrow_kernels.hip.h) -- the
// resident key, the staging of the host entry points, the launches and what the last launch of each did.  Owned by its
// engine (Engine::packing), every launch on the engine's stream.
struct Engine;
struct Packing {
    Engine* e = nullptr;                 // set in Engine::create
    DeviceBuffer<int8_t> key;            // the packing key's balanced base-256 digit planes in MFMA B-fragment order
    fhe_packing_params_t pp{0, 0};       // its decomposition
    DeviceBuffer<int8_t> digits;         // the batch's digit fragments; same reuse rules as PipeLane::digits: zeroed at allocation, grown, rows past the batch never read
    DeviceBuffer<uint64_t> pack_in, pack_out;       // staging of fhe_engine_pack_lwes (host ciphertexts)
    uint32_t pack_last[5] = {0, 0, 0, 0, 0};        // fhe_engine_packing_info: ran, MT, K chunks, K steps per chunk, K steps
    DeviceBuffer<uint64_t> unpack_in, unpack_out;   // staging of fhe_engine_unpack_glwes; unpack_out also of fhe_engine_unpack_narrow
    uint32_t unpack_last[4] = {0, 0, 0, 0};         // fhe_engine_unpack_info: ran, rows, workgroups, refreshed
    DeviceBuffer<uint64_t> narrow_in, narrow_out;   // staging of fhe_engine_narrow_glwes; narrow_in also of fhe_engine_unpack_narrow
    uint32_t narrow_last[5] = {0, 0, 0, 0, 0};      // fhe_engine_narrow_info: ran, kernel (FHE_NARROW_KERNEL_*), list words / rows / GLWE words, workgroups, bits
    void pack_info(uint32_t out[5]) const { std::copy(pack_last, pack_last + 5, out); }
    void unpack_info(uint32_t out[4]) const { std::copy(unpack_last, unpack_last + 4, out); }
    void narrow_info(uint32_t out[5]) const { std::copy(narrow_last, narrow_last + 5, out); }

    int load_key(const fhe_packing_params_t& pp, const uint64_t* pksk);
    int pack_dev(const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes);
    int pack_host(const uint64_t* cts, uint32_t count, uint64_t* glwes);
    int extract_dev(const char* who, uint32_t k, uint32_t N, const uint64_t* d_glwes, uint32_t first, uint32_t count, uint64_t* d_cts, uint32_t* chunks = nullptr);
    int unpack_dev(const uint64_t* d_glwes, uint32_t first, uint32_t count, int refresh, uint64_t* d_cts);
    int unpack_host(const uint64_t* glwes, uint32_t first, uint32_t count, int refresh, uint64_t* cts);
    int narrow_dev(const uint64_t* d_glwes, uint32_t held, uint32_t bits, uint64_t* d_narrow);
    int narrow_host(const uint64_t* glwes, uint32_t held, uint32_t bits, uint64_t* narrow);
    int widen_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint64_t* d_glwes);
    int widen_shape_dev(const char* who, uint32_t k, uint32_t N, const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint64_t* d_glwes);
    int unpack_narrow_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int refresh, uint64_t* d_cts);
    int unpack_narrow_host(const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int refresh, uint64_t* cts);

    // Ring packing (ring_packing.h, ring_packing_kernels.hip.h): a second route to the same packed GLWEs, through log2(N)
    // automorphism keys.  With a matrix key loaded as well, the refresh gate judges by the matrix key's pair, as before.
    DeviceBuffer<uint32_t> ring_key;     // the automorphism keys' transformed digit planes [log2 N][k L][k+1][8][N]
    fhe_packing_params_t ring_pp{0, 0};
    DeviceBuffer<uint32_t> ring_tw;      // twiddles of the key's N: N forward, then N inverse
    uint32_t ring_n_inv = 0;
    DeviceBuffer<uint64_t> ring_slots;   // the leaves and the nodes that replace them: count x [k+1][N]
    DeviceBuffer<unsigned char> ring_tmp;   // one batch of merges: transformed digits, permuted bodies, lifted products
    uint64_t ring_last[5] = {0, 0, 0, 0, 0};   // fhe_engine_ring_pack_info: ran, tree levels, automorphism keyswitches, launches, scratch bytes
    int load_ring_key(const fhe_packing_params_t& pp, const uint64_t* key);
    int ring_pack_dev(const uint64_t* d_cts, uint32_t count, uint64_t* d_glwes);
    int ring_pack_host(const uint64_t* cts, uint32_t count, uint64_t* glwes);
    int ring_ntt_host(uint32_t N, int inverse, uint32_t* polys, uint32_t count);   // the device transform on its own, host arrays
};

// Transciphering (transcipher.h, transcipher_kernels.hip.h; members in transcipher_dev.hip): the resident encrypted key bits
// of one stream-cipher key and the round ring of up to max_streams strings encrypted under it, each with its own IV,
// advancing in lockstep -- one ks_pbs level per round for all of them.  Owned by its engine (Engine::transciphers), every
// launch on the engine's stream.
struct Transcipher {
    Engine* e = nullptr;
    uint32_t cipher = 0, max_streams = 0, bits = 0;
    uint32_t n_streams = 0;             // 0 until begin()
    int32_t round = 0;                  // the next round: TC_WARMUP_ROUNDS after begin(), then one more per 8 bytes
    DeviceBuffer<uint64_t> key;         // L rows K_1 .. K_L
    DeviceBuffer<uint64_t> ring;        // tc_ring_rows(max_streams) rows
    DeviceBuffer<uint64_t> pbs_in;      // the gather's output: max_streams x 256 rows
    DeviceBuffer<uint32_t> tables;      // and its table indices
    DeviceBuffer<uint8_t> ivs, data;    // the streams' clear IVs; the clear cipher bytes of the current next()
    DeviceBuffer<uint64_t> out;         // staging of next() with a host destination
    uint32_t lut_of[20] = {};           // table number (transcipher.h) -> the engine's table index, through lut_upload_dedup
    uint32_t warm_rounds = 0, data_rounds = 0;   // since begin()
    uint64_t pbs_rows = 0;              // lookups since begin(), all streams, the refresh included
    // per-phase device times of the data rounds since begin(), measured only when `timed` (each round then ends in a
    // synchronisation): gather, ks_pbs, apply in ms, and the rounds measured
    bool timed = false;
    double phase_ms[3] = {0, 0, 0};
    uint32_t timed_rounds = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};

    static int create(Engine& e, uint32_t cipher, const uint64_t* key_cts, uint32_t max_streams, Transcipher** out);
    ~Transcipher();
    int begin(const uint8_t* ivs_host, uint32_t streams);
    int next(const uint8_t* data_host, uint32_t n_bytes, int refresh, uint64_t* out_host, uint64_t* d_out);
    int run_round(uint32_t rows, uint32_t n_bytes, uint32_t m, uint64_t* d_blocks);
    void info(uint32_t out[8]) const;
};

// Casting keys (cast.h, cast_kernels.hip.h; members in cast_dev.hip): one resident key from a source client's big key to
// this engine's big or small key, in the matrix-core keyswitch's digit planes, with the buffers of its casts -- the
// digit fragments, the keyswitched rows, the bodies gathered from packed GLWEs, the staging of the host forms.  An engine
// serves many source clients: owned by its engine (Engine::cast_keys), every launch on the engine's stream.
struct CastKey {
    Engine* e = nullptr;
    fhe_cast_params_t cp{};
    int32_t shift = 0;                  // cast_rshift
    uint32_t in_dim = 0, out_size = 0;  // source k N; out_dim + 1 words of a keyswitched row
    DeviceBuffer<int8_t> key;           // B-fragment planes
    DeviceBuffer<int8_t> digits;        // A fragments; same reuse rules as PipeLane::digits
    DeviceBuffer<uint64_t> rows;        // the keyswitched rows, then the regrouped ones behind them
    DeviceBuffer<uint64_t> bodies;      // B[j_b] of a packed batch, one word per block: what the product reads as bodies
    DeviceBuffer<uint64_t> lwes;        // the extracted rows of a packed batch when the fused digit kernel is off
    DeviceBuffer<uint64_t> glwes;       // a narrow list widened to the source's full GLWEs (cast_narrow_dev)
    DeviceBuffer<uint32_t> idx;         // the follow-up table's index, once per row of the largest cast so far
    DeviceBuffer<unsigned char> meta;   // regrouping: offsets, sources, weights, constants of lincomb_kernel
    DeviceBuffer<uint64_t> in, out;     // staging of the host forms
    bool fused = true;                  // packed inputs through cast_decompose_glwe_kernel
    uint32_t group = 1;                 // source blocks per destination block (fhe_cast_key_set_group)
    uint32_t meta_count = 0;            // the batch `meta` was written for
    uint32_t lut = 0;                   // the follow-up table's id on the engine, once uploaded
    bool lut_ready = false;
    uint32_t last = 0;                  // fhe_cast_key_info[7]
    double v_in = 1.0;                  // what the source blocks are declared to carry, in the source's nominal units (gate)

    static int create(Engine& e, const fhe_cast_params_t& cp, const uint64_t* key, CastKey** out);
    int set_group(uint32_t group);
    int gate(const char* who) const;    // the follow-up lookup's input against the PBS-input budget (cast_noise)
    int keyswitch_dev(const uint64_t* d_src, uint32_t first, uint32_t count, bool packed, uint64_t* d_rows);
    int cast_dev(const uint64_t* d_src, uint32_t first, uint32_t count, bool packed, int mode, uint64_t* d_out);
    int cast_host(const uint64_t* src, uint32_t first, uint32_t count, bool packed, int mode, uint64_t* out);
    // blocks first .. first + count - 1 of the source's narrow list of `held` blocks: widened on the device (glwe_widen_kernel at
    // the source's shape), then cast as packed GLWEs
    int cast_narrow_dev(const uint64_t* d_narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* d_out);
    int cast_narrow_host(const uint64_t* narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count, int mode, uint64_t* out);
    int digits_host(const uint64_t* src, uint32_t first, uint32_t count, bool packed, int8_t* out, size_t* bytes);
    void info(uint32_t out[8]) const;
};

struct Engine {
    std::recursive_mutex mu;      // taken by every C ABI entry point that touches this engine (c_api.cpp, LOCK_ENGINE)
    fhe_params_t p{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::map<std::vector<uint64_t>, uint32_t> lut_dedup;
    std::vector<hipEvent_t> ring;   // 4 events per recorded ks_pbs call (timing_events)
    size_t ring_used = 0;           // calls recorded since the last reset
    const BrVariant* variant = nullptr;       // layout used up to one LWE per CU
    const BrVariant* variant_large = nullptr; // same Fourier-key layout, used for larger batches (may equal variant)
    int cu_count = 256;
    uint32_t max_grid[3] = {0x7FFFFFFFu, 65535u, 65535u};   // hipDeviceProp_t::maxGridSize, read in Engine::create: no launch passes a larger grid dimension
    // The spans of a grid dimension that grows with a batch or a key size (grid_spans.h); axis 0, 1, 2 = x, y, z.
    GridSpans spans(uint64_t count, int axis) const { return grid_spans(count, max_grid[axis]); }
    // A dimension that a documented batch limit keeps within one launch: anything else is refused, never launched.
    int one_span(const char* who, uint64_t count, int axis) const {
        if (spans(count, axis).spans == 1) return 0;
        return fail(std::string(who) + ": grid." + "xyz"[axis] + " = " + std::to_string(count) + " does not fit one launch (the device allows " +
                    std::to_string(max_grid[axis]) + ")");
    }
    EngineSettings cfg;                       // defaults, environment (Engine::create) and the fhe_engine_set_* setters: engine_settings.h
    int pipeline = 0;                         // ks_pbs_dev throughput modes: 1 = keyswitch of call k+1 in the shadow of the blind rotation of call k; 2 = whole calls overlapped on pipe.width lanes
    Pipeline pipe;                           // streams, events, buffers and hazard records of the throughput modes; lane 0's buffers serve every serial call
    int sync_all_streams() { return pipe.wait_all(stream); }
    // A call outside the throughput modes whose buffers their calls may still touch on other streams: wait for every stream
    // and end the pipelined run, like any serial call.
    int leave_pipelined_run() {
        if (!pipeline) return 0;
        if (sync_all_streams()) return 1;
        pipe.end_run();
        return 0;
    }
    // Grow a buffer that launches in flight on any of the engine's streams may still read: they finish before the old
    // allocation goes.  Nothing can be reading an empty buffer, so a first allocation does not wait.
    template <class T>
    int reserve_idle(DeviceBuffer<T>& b, size_t need) {
        if (b.bytes >= need) return 0;
        if (b.ptr && sync_all_streams()) return 1;
        return b.reserve(need);
    }
    int shadow_fit = -1;                      // -1 unknown, else whether a 64-VGPR wave fits next to the rotation's

    // resident keys / tables
    DeviceBuffer<uint32_t> d_ksk_packed; // [rows/4][8][n+1] byte planes for keyswitch_dot4_kernel
    DeviceBuffer<uint64_t> d_ksk_rowsum; // [kN / KS_IC][n+1] sums of every tile's key rows (bias removal)
    DeviceBuffer<int8_t> d_ksk_mfma;  // balanced base-256 digit planes of the KSK in MFMA B-fragment order (ks_mfma_kernels.hip.h)
    DeviceBuffer<double> d_fbsk;
    DeviceBuffer<double> d_fbsk_dense;       // the same key in the dense wide kernel's Fourier order (N = 1024, k = 2 only)
    DeviceBuffer<uint64_t> d_luts;
    uint32_t n_luts = 0;

    // staging / scratch (grown on demand)
    DeviceBuffer<uint64_t> d_in, d_out, d_pool;   // the small ciphertexts between keyswitch and rotation: pipe.lane[q].small
    DeviceBuffer<uint32_t> d_idx;
    DeviceBuffer<unsigned char> d_meta;
    DeviceBuffer<uint64_t> d_compact;   // a compact ciphertext list on its way to compact_expand_kernel
    // Blind-rotation workspace, shared by three paths of blind_rotate.hip: the large-N kernel's per-LWE HBM workspace
    // (rotate_large), the prepared GGSWs of the multi-bit combined path (rotate_multibit_combined), and the prepared GGSWs
    // followed by the rotation workspace of the multi-bit two-kernel path (rotate_multibit_two_kernel, at most
    // cfg.multibit_workspace_cap bytes).  Contract: one launch sequence at a time, on the engine's stream -- a path reserves
    // it, launches everything that reads or writes it on `stream`, and returns; stream order then separates it from the
    // next user.  No launch on a pipeline lane's own stream may touch it (the overlapped path takes none of the three).
    DeviceBuffer<unsigned char> d_ws;
    DeviceBuffer<uint32_t> d_slot_exp;   // multi-bit two-kernel path: exponent of w = e^{i pi / N} each Fourier slot evaluates at
    MultiCuRuntime multi_cu;            // the 8-CU clusters and the whole-XCD kernel: their workspace, control block and status checks (blind_rotate.h)
    // what the last launch_keyswitch launched (fhe_engine_keyswitch_info; recorded only, read by no decision): kernel
    // (FHE_KS_KERNEL_*), row tiles / samples per workgroup, K chunks (grid.z), K steps / input coefficients per chunk, K steps / in_dim
    uint32_t ks_last[5] = {0, 0, 0, 0, 0};
    Packing packing;                    // the packed-ciphertext family: pack, unpack, narrow (packing_dev.hip)
    DeviceBuffer<uint32_t> refresh_idx; // refresh_rows_dev's table indices: the identity table's id, once per row of the largest refresh so far
    std::vector<std::unique_ptr<Transcipher>> transciphers;   // fhe_transcipher_create .. fhe_transcipher_destroy, or the engine's end
    std::vector<std::unique_ptr<CastKey>> cast_keys;          // fhe_cast_key_create .. fhe_cast_key_destroy, or the engine's end

    static int create(const fhe_params_t& p, int device, Engine** out);
    ~Engine();
    int use();
    int set_variant(int logR);   // blind_rotate.hip, like every member below that names a variant's kernel
    int allow_rotate_lds();   // hipFuncAttributeMaxDynamicSharedMemorySize of the variants' rotation kernels
    int load_keys(const uint64_t* bsk_std, const uint64_t* ksk);
    int load_seeded_keys(const uint8_t ksk_seed[16], const uint64_t* ksk_bodies, const uint8_t bsk_seed[16], const uint64_t* bsk_bodies,
                         uint64_t* bsk_std_out, uint64_t* ksk_out);
    int expand_seeded_lwe(const uint8_t* seeds, const uint64_t* bodies, uint32_t count, uint64_t* d_out, uint64_t* host_out);
    int expand_compact_list(const uint64_t* list, uint32_t count, uint64_t* d_out, uint64_t* host_out);
    int expand_compact_list_dev(const uint64_t* d_list, uint32_t count, uint64_t* d_out);
    int generate_keys(const uint64_t* glwe_sk, const uint64_t* small_sk, const uint8_t seed[32],
                      uint64_t* bsk_std_out, uint64_t* ksk_out);
    int install_keys(DeviceBuffer<uint64_t>&& d_ksk_std, DeviceBuffer<uint64_t>&& d_bsk_std);
    int convert_polys(const uint64_t* d_std, double* d_out, uint32_t n_polys);
    int convert_dense_key(const uint64_t* d_std, uint32_t n_polys);   // d_fbsk_dense, where variant_large has a dense kernel
    int probe_slot_exponents();
    uint64_t fill_accumulator(const uint64_t* table, std::vector<uint64_t>& acc) const { return fhe::fill_accumulator(p, table, acc); }
    int lut_upload_dedup(const std::vector<uint64_t>& acc, uint32_t* id);   // same contents -> same id
    int set_stream(hipStream_t s, bool use_own);   // launch on a caller-owned stream (e.g. the framework's current stream)
    int lut_upload(const uint64_t* acc, uint32_t* id);
    int lut_download(uint32_t id, uint64_t* acc);
    int ensure_batch(uint32_t count);
    int timing_events(hipEvent_t*& e4);   // the next recorded call's: keyswitch start / end, blind rotation start / end
    int check_lut_idx(const uint32_t* lut_idx, uint32_t count) const;

    int launch_keyswitch(const uint64_t* d_big, uint64_t* d_sm, uint32_t count, DeviceBuffer<int8_t>& digits, hipStream_t on = nullptr, bool shadow = false);
    int launch_blind_rotate(const uint64_t* d_sm, const uint32_t* d_lut_idx, uint64_t* d_big, uint32_t count, hipStream_t on = nullptr, bool two_per_cu = false,
                            bool one_workgroup_only = false);   // never a kernel that needs several workgroups resident at once (MultiCuRuntime::settle's re-run)
    bool shadow_keyswitch_fits();
    int refresh_rows_dev(uint64_t* d_cts, uint32_t count);   // one ks_pbs level with the identity table, in place: what both unpack forms and Transcipher::next end with
    uint32_t rotate_registers() const;             // VGPRs of variant's rotation kernel, 0 if unknown
    void keyswitch_info(uint32_t info[6]) const;   // ks_last and the register count shadow_keyswitch_fits judges by; changes nothing
    int ks_pbs_dev(const uint64_t* d_big_in, const uint32_t* d_lut_idx, uint64_t* d_big_out, uint32_t count, bool allow_pipeline = false);
    int ks_pbs_host(const uint64_t* in, const uint32_t* lut_idx, uint64_t* out, uint32_t count);
    int keyswitch_host(const uint64_t* in, uint64_t* out_small, uint32_t count);
    int pbs_host(const uint64_t* in_small, const uint32_t* lut_idx, uint64_t* out, uint32_t count);
    int pbs_ks_host(const uint64_t* in_small, const uint32_t* lut_idx, uint64_t* out_small, uint32_t count);
    int lincomb_dev(const uint64_t* d_pool, const uint32_t* d_off, const uint32_t* d_src,
                    const int32_t* d_coeff, const uint64_t* d_cst, uint64_t* d_out, uint32_t jobs);
    // the same on rows of any length (the casting keys combine keyswitched rows, small ones too)
    int lincomb_rows_dev(const uint64_t* d_pool, const uint32_t* d_off, const uint32_t* d_src, const int32_t* d_coeff, const uint64_t* d_cst,
                         uint64_t* d_out, uint32_t jobs, uint32_t row_words);
    // `instances` copies of a plan level at once (lincomb_batch_kernel); strides in ciphertext rows
    int lincomb_batch_dev(const uint64_t* d_pool, const uint32_t* d_off, const uint32_t* d_src, const int32_t* d_coeff,
                          const uint64_t* d_cst, uint64_t* d_out, uint32_t jobs, uint32_t instances, uint32_t src_slot, uint32_t src_inst,
                          uint32_t out_job, uint32_t out_inst, const uint32_t* d_lut_in, uint32_t* d_lut_out);
    int restride_dev(const uint64_t* d_in, uint64_t* d_out, uint32_t slots, uint32_t instances, uint32_t in_slot, uint32_t in_inst,
                     uint32_t out_slot, uint32_t out_inst);
    int lincomb_host(const uint64_t* pool, uint32_t pool_count, const uint32_t* off, const uint32_t* src,
                     const int32_t* coeff, const uint64_t* cst, uint64_t* out, uint32_t jobs);
    // the three transcipher kernels on host arrays, one launch each (transcipher_dev.hip): what tests compare with transcipher.cpp
    int transcipher_init_host(uint32_t cipher, uint32_t S, const uint64_t* key, const uint8_t* ivs, uint64_t* ring);
    int transcipher_gather_host(uint32_t cipher, uint32_t S, int32_t round, uint32_t rows, const uint64_t* ring, const uint64_t* key, const uint8_t* ivs,
                                const uint8_t* data, uint32_t n_bytes, uint32_t m, uint64_t* pbs_in, uint32_t* tables);
    int transcipher_apply_host(uint32_t cipher, uint32_t S, int32_t round, const uint64_t* ring, uint32_t n_bytes, uint32_t m, uint64_t* out);
    int last_kernel_ms(float ms[2]);
    int kernel_times(double total_ms[2], uint32_t* calls, bool reset);
    int synchronize();
};

// compact_pk.cpp: k*N if it is a power of two (the dimension a compact public key works in), else 0; key generation
struct Seed256;
size_t compact_dim(const fhe_params_t& p);
int compact_pk_generate(const fhe_params_t& p, const uint64_t* big_sk, const Seed256& seed, uint64_t* pk, int threads);

int params_supported(const fhe_params_t& p);   // 0, or 1 with the reason in fhe_last_error (no device needed)
// client.cpp: the same answer for a packing keyswitch decomposition on a parameter set
int packing_params_check(const fhe_params_t& p, const fhe_packing_params_t& pp);
// client.cpp: out[0] variance of a raw extracted block of a packed PBS output in nominal units, out[1] the PBS-input budget
void packing_unpack_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, double out[2]);
// client.cpp: the same block after the GLWE was narrowed to `bits` (glwe_narrow.h): out[0] its variance in nominal units,
// out[1] the PBS-input budget, out[2] log2 of the probability that the client decodes such a coefficient wrongly
void narrow_noise(const fhe_params_t& p, const fhe_packing_params_t& pp, uint32_t bits, double out[3]);

}  // namespace fhe

struct fhe_plan;
struct fhe_engine {
    fhe::Engine* impl;
    // plans of the one-call string operations (fhe_str_eq ...), most recently used first: building a
    // plan and allocating its pool costs milliseconds, the same (op, capacities, clear pattern) recurs
    std::vector<std::pair<std::string, fhe_plan*>> str_plans;
};
