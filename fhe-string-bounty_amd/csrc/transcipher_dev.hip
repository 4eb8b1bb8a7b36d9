// transcipher_dev.hip -- fhe::Transcipher (engine.h): the launches of transcipher_kernels.hip.h around Engine::ks_pbs_dev.
//
// A round is: transcipher_gather_kernel (S x rows lookup inputs and their table indices from ring slots r - 1 and r - 2
// and the resident key rows) -> ks_pbs_dev straight into ring slot r mod 4 -> on data rounds transcipher_apply_kernel
// (the round's <= 8 characters of every stream into the destination string).  Everything is ordered on the engine's
// stream; nothing synchronises except a call with a host destination, and the per-phase timing when it is switched on.
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "transcipher_kernels.hip.h"

namespace fhe {

static_assert(TC_MAX_TABLES == sizeof(Transcipher::lut_of) / sizeof(uint32_t), "engine.h sizes lut_of without transcipher.h");

namespace {

TcDeviceShape device_shape(const TcShape& sh) { return TcDeviceShape{sh.big, sh.bits, sh.cipher, sh.S, sh.delta}; }

int shape_of(const Engine& e, uint32_t cipher, uint32_t S, TcShape* sh) {
    if (const char* why = tc_shape(e.p, cipher, S, sh)) return fail(why);
    return 0;
}

int launch_init(Engine& e, const TcShape& sh, const uint64_t* d_key, const uint8_t* d_ivs, uint64_t* d_ring) {
    hipLaunchKernelGGL(transcipher_init_kernel, dim3(sh.S * 2 * TC_STATE_ROWS), dim3(256), 0, e.stream, device_shape(sh), d_key, d_ivs, d_ring);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_gather(Engine& e, const TcShape& sh, int32_t round, uint32_t rows, const uint64_t* d_ring, const uint64_t* d_key, const uint8_t* d_ivs,
                  const uint8_t* d_data, uint32_t n_bytes, uint32_t m, const uint32_t* lut_of, uint64_t* d_pbs_in, uint32_t* d_tables) {
    TcGatherArgs a{};
    a.sh = device_shape(sh);
    a.ring = d_ring; a.key = d_key; a.ivs = d_ivs; a.data = rows == TC_DATA_ROWS ? d_data : nullptr;
    a.pbs_in = d_pbs_in; a.tables = d_tables;
    a.round = round; a.rows = rows; a.n_bytes = n_bytes; a.m = m;
    for (uint32_t t = 0; t < TC_MAX_TABLES; t++) a.lut_of[t] = lut_of ? lut_of[t] : t;
    hipLaunchKernelGGL(transcipher_gather_kernel, dim3(sh.S * rows), dim3(256), 0, e.stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_apply(Engine& e, const TcShape& sh, int32_t round, const uint64_t* d_ring, uint32_t n_bytes, uint32_t m, uint64_t* d_out) {
    const uint32_t chars = n_bytes - 8 * m < 8 ? n_bytes - 8 * m : 8;          // 8 m < n_bytes: checked by the callers
    hipLaunchKernelGGL(transcipher_apply_kernel, dim3(sh.S * chars * tc_blocks_per_char(sh)), dim3(256), 0, e.stream, device_shape(sh), d_ring, d_out, round,
                       n_bytes, m, chars);
    HIP_TRY(hipGetLastError());
    return 0;
}

int round_checks(int32_t round, uint32_t rows, uint32_t n_bytes, uint32_t m, bool apply) {
    if (round < 0 || round > (1 << 24)) return fail("transcipher: round out of range");
    if (rows != TC_STATE_ROWS && rows != TC_DATA_ROWS) return fail("transcipher: a round has 192 or 256 rows");
    if (apply && round < (int32_t)TC_WARMUP_ROUNDS) return fail("transcipher: a warm-up round has no keystream rows");
    if (apply && (uint64_t)8 * m >= n_bytes) return fail("transcipher: round m of a call starts at byte 8 m, past the call's bytes");
    return 0;
}

}  // namespace

// ---- the kernels on host arrays: one launch each, what tests/test_gpu_transcipher.py compares with transcipher.cpp ----
int Engine::transcipher_init_host(uint32_t cipher, uint32_t S, const uint64_t* key, const uint8_t* ivs_host, uint64_t* ring) {
    if (use()) return 1;
    TcShape sh;
    if (shape_of(*this, cipher, S, &sh) || leave_pipelined_run()) return 1;
    const size_t L = stream_key_bits(cipher), ring_bytes = tc_ring_rows(S) * sh.big * 8;
    DeviceBuffer<uint64_t> d_key, d_ring;
    DeviceBuffer<uint8_t> d_ivs;
    if (d_key.alloc(L * sh.big * 8) || d_ring.alloc(ring_bytes) || d_ivs.alloc(S * L / 8)) return 1;
    HIP_TRY(hipMemcpyAsync(d_key, key, L * sh.big * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_ivs, ivs_host, S * L / 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_ring, ring, ring_bytes, hipMemcpyHostToDevice, stream));      // the rows the kernel leaves alone come back as they were
    if (launch_init(*this, sh, d_key, d_ivs, d_ring)) return 1;
    HIP_TRY(hipMemcpyAsync(ring, d_ring, ring_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int Engine::transcipher_gather_host(uint32_t cipher, uint32_t S, int32_t round, uint32_t rows, const uint64_t* ring, const uint64_t* key, const uint8_t* ivs_host,
                                    const uint8_t* data, uint32_t n_bytes, uint32_t m, uint64_t* pbs_in, uint32_t* tables) {
    if (use()) return 1;
    TcShape sh;
    if (shape_of(*this, cipher, S, &sh) || round_checks(round, rows, n_bytes, m, false) || leave_pipelined_run()) return 1;
    const size_t L = stream_key_bits(cipher), ring_bytes = tc_ring_rows(S) * sh.big * 8, out_rows = (size_t)S * rows;
    const bool with_data = rows == TC_DATA_ROWS && data && n_bytes;
    DeviceBuffer<uint64_t> d_key, d_ring, d_in;
    DeviceBuffer<uint8_t> d_ivs, d_data;
    DeviceBuffer<uint32_t> d_tables;
    if (d_key.alloc(L * sh.big * 8) || d_ring.alloc(ring_bytes) || d_ivs.alloc(S * L / 8) || d_in.alloc(out_rows * sh.big * 8) || d_tables.alloc(out_rows * 4)) return 1;
    if (with_data && d_data.alloc((size_t)S * n_bytes)) return 1;
    HIP_TRY(hipMemcpyAsync(d_key, key, L * sh.big * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_ivs, ivs_host, S * L / 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_ring, ring, ring_bytes, hipMemcpyHostToDevice, stream));
    if (with_data) HIP_TRY(hipMemcpyAsync(d_data, data, (size_t)S * n_bytes, hipMemcpyHostToDevice, stream));
    if (launch_gather(*this, sh, round, rows, d_ring, d_key, d_ivs, with_data ? d_data.ptr : nullptr, n_bytes, m, nullptr, d_in, d_tables)) return 1;
    HIP_TRY(hipMemcpyAsync(pbs_in, d_in, out_rows * sh.big * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(tables, d_tables, out_rows * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int Engine::transcipher_apply_host(uint32_t cipher, uint32_t S, int32_t round, const uint64_t* ring, uint32_t n_bytes, uint32_t m, uint64_t* out) {
    if (use()) return 1;
    TcShape sh;
    if (shape_of(*this, cipher, S, &sh) || round_checks(round, TC_DATA_ROWS, n_bytes, m, true) || leave_pipelined_run()) return 1;
    const size_t ring_bytes = tc_ring_rows(S) * sh.big * 8, out_bytes = (size_t)S * n_bytes * tc_blocks_per_char(sh) * sh.big * 8;
    DeviceBuffer<uint64_t> d_ring, d_out;
    if (d_ring.alloc(ring_bytes) || d_out.alloc(out_bytes)) return 1;
    HIP_TRY(hipMemcpyAsync(d_ring, ring, ring_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_out, out, out_bytes, hipMemcpyHostToDevice, stream));         // the blocks of other rounds come back as they were
    if (launch_apply(*this, sh, round, d_ring, n_bytes, m, d_out)) return 1;
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

// ---- Transcipher ------------------------------------------------------------------------------------------------------
int Transcipher::create(Engine& e, uint32_t cipher, const uint64_t* key_cts, uint32_t max_streams, Transcipher** out) {
    if (e.use()) return 1;
    TcShape sh;
    if (shape_of(e, cipher, max_streams, &sh)) return 1;
    if (!e.d_fbsk) return fail("transcipher: the engine has no server keys loaded");
    if (e.leave_pipelined_run()) return 1;
    std::unique_ptr<Transcipher> t(new Transcipher());
    t->e = &e; t->cipher = cipher; t->max_streams = max_streams; t->bits = sh.bits;
    const size_t L = stream_key_bits(cipher), row = (size_t)sh.big * 8;
    if (t->key.alloc(L * row) || t->ring.alloc(tc_ring_rows(max_streams) * row) || t->pbs_in.alloc((size_t)max_streams * TC_DATA_ROWS * row) ||
        t->tables.alloc((size_t)max_streams * TC_DATA_ROWS * 4) || t->ivs.alloc(max_streams * L / 8))
        return 1;
    HIP_TRY(hipMemcpyAsync(t->key, key_cts, L * row, hipMemcpyHostToDevice, e.stream));
    const uint32_t values = e.p.msg_mod * e.p.carry_mod, n_tables = TC_TABLE_G + 2 * sh.bits;
    std::vector<uint64_t> table(values), acc;
    for (uint32_t k = 0; k < n_tables; k++) {
        for (uint32_t v = 0; v < values; v++) table[v] = tc_table_value(k, v);
        e.fill_accumulator(table.data(), acc);
        if (e.lut_upload_dedup(acc, &t->lut_of[k])) return 1;
    }
    HIP_TRY(hipStreamSynchronize(e.stream));                      // the caller's key rows are free again
    *out = t.get();
    e.transciphers.push_back(std::move(t));
    return 0;
}

Transcipher::~Transcipher() {
    for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
}

int Transcipher::begin(const uint8_t* ivs_host, uint32_t streams) {
    if (e->use()) return 1;
    if (streams == 0 || streams > max_streams)
        return fail("transcipher: begin with " + std::to_string(streams) + " streams, the object was created for 1 .. " + std::to_string(max_streams));
    if (e->leave_pipelined_run()) return 1;
    TcShape sh;
    if (shape_of(*e, cipher, streams, &sh)) return 1;
    n_streams = 0;                                                // a failure below leaves the object without a run, not with half of one
    HIP_TRY(hipMemcpyAsync(ivs, ivs_host, streams * stream_key_bits(cipher) / 8, hipMemcpyHostToDevice, e->stream));
    if (launch_init(*e, sh, key, ivs, ring)) return 1;
    n_streams = streams;
    round = 0; warm_rounds = data_rounds = 0; pbs_rows = 0;
    timed_rounds = 0; phase_ms[0] = phase_ms[1] = phase_ms[2] = 0;
    for (uint32_t r = 0; r < TC_WARMUP_ROUNDS; r++) {
        if (run_round(TC_STATE_ROWS, 0, 0, nullptr)) { n_streams = 0; return 1; }
        warm_rounds++;
    }
    return 0;
}

// Round `round` of every stream: gather, one ks_pbs level into the round's ring slot, and on a data round the block sums of
// characters 8 m .. of the call into d_blocks.
int Transcipher::run_round(uint32_t rows, uint32_t n_bytes, uint32_t m, uint64_t* d_blocks) {
    TcShape sh;
    if (shape_of(*e, cipher, n_streams, &sh)) return 1;
    const bool data_round = rows == TC_DATA_ROWS, time_it = timed && data_round;
    if (time_it)
        for (auto& x : ev)
            if (!x) HIP_TRY(hipEventCreate(&x));
    const uint32_t count = n_streams * rows;
    if (time_it) HIP_TRY(hipEventRecord(ev[0], e->stream));
    if (launch_gather(*e, sh, round, rows, ring, key, ivs, data, n_bytes, m, lut_of, pbs_in, tables)) return 1;
    if (time_it) HIP_TRY(hipEventRecord(ev[1], e->stream));
    if (e->ks_pbs_dev(pbs_in, tables, ring + tc_slot_row(n_streams, round) * sh.big, count)) return 1;
    if (time_it) HIP_TRY(hipEventRecord(ev[2], e->stream));
    if (data_round && launch_apply(*e, sh, round, ring, n_bytes, m, d_blocks)) return 1;
    if (time_it) {
        HIP_TRY(hipEventRecord(ev[3], e->stream));
        HIP_TRY(hipEventSynchronize(ev[3]));
        for (int ph = 0; ph < 3; ph++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev[ph], ev[ph + 1]));
            phase_ms[ph] += ms;
        }
        timed_rounds++;
    }
    pbs_rows += count;
    round++;
    return 0;
}

int Transcipher::next(const uint8_t* data_host, uint32_t n_bytes, int refresh, uint64_t* out_host, uint64_t* d_out) {
    if (e->use()) return 1;
    if (n_streams == 0) return fail("transcipher: next before begin");
    if (n_bytes == 0) return 0;
    if (n_bytes > (1u << 20)) return fail("transcipher: at most 2^20 bytes per stream in one call");
    if (!out_host == !d_out) return fail("transcipher: exactly one of a host and a device destination");
    if (e->leave_pipelined_run()) return 1;
    TcShape sh;
    if (shape_of(*e, cipher, n_streams, &sh)) return 1;
    const uint32_t rounds = (n_bytes + 7) / 8;
    if ((int64_t)round + rounds > (1 << 24)) return fail("transcipher: keystream exhausted (2^24 rounds)");
    const size_t blocks = (size_t)n_streams * n_bytes * tc_blocks_per_char(sh), row = (size_t)sh.big * 8;
    if (blocks > 0x7FFFFFFFull) return fail("transcipher: too many blocks for one call");
    if (e->reserve_idle(data, (size_t)n_streams * n_bytes)) return 1;
    if (out_host && e->reserve_idle(out, blocks * row)) return 1;
    uint64_t* d_blocks = out_host ? out.ptr : d_out;
    HIP_TRY(hipMemcpyAsync(data, data_host, (size_t)n_streams * n_bytes, hipMemcpyHostToDevice, e->stream));
    for (uint32_t m = 0; m < rounds; m++) {
        if (run_round(TC_DATA_ROWS, n_bytes, m, d_blocks)) return 1;
        data_rounds++;
    }
    if (refresh) {
        if (e->refresh_rows_dev(d_blocks, (uint32_t)blocks)) return 1;
        pbs_rows += blocks;
    }
    if (!out_host) return 0;
    HIP_TRY(hipMemcpyAsync(out_host, d_blocks, blocks * row, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return e->multi_cu.check();
}

void Transcipher::info(uint32_t o[8]) const {
    o[0] = cipher; o[1] = max_streams; o[2] = n_streams; o[3] = warm_rounds; o[4] = data_rounds;
    o[5] = (uint32_t)(pbs_rows & 0xFFFFFFFFu); o[6] = (uint32_t)(pbs_rows >> 32);
    o[7] = 8 * data_rounds;                                        // the keystream byte the next call starts at
}

}  // namespace fhe
