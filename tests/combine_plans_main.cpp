// combine_plans_main.cpp -- the planner units (csrc/circuit.cpp, fhe_string.cpp, the str_*.cpp units behind str_ops.h,
// regex.cpp, str_op_name.cpp; count_ops.h and radix_ops.h are headers) linked into a stand-alone program that builds
// every plan name that combines results -- the bit logic, select, select_count, the count arithmetic and comparisons with
// an encrypted and with a clear second operand -- offline at capacities and bounds 1 .. 9 and the count names at three-digit
// bounds as well, on 2-bit and on 4-bit blocks, and finalises each plan for one and for two ranks.  It prints one line per plan: its info, or the refusal.  Compiled
// under the host sanitizers by tests/test_combine_host.py; nothing is loaded into Python and no device is touched: a
// circuit without an engine never reaches the engine's device calls, which are stubs below, and the tables' accumulators
// -- read only when a plan runs -- are left empty.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "circuit.h"
#include "str_op_name.h"

namespace fhe {

static std::string g_error;
int fail(const std::string& msg) {
    g_error = msg;
    return 1;
}
uint64_t fill_accumulator(const fhe_params_t& p, const uint64_t* table, std::vector<uint64_t>& acc) {
    acc.assign(1, 0);
    return *std::max_element(table, table + (size_t)p.msg_mod * p.carry_mod);
}
void fill_accumulator_torus(const fhe_params_t&, const uint64_t*, std::vector<uint64_t>& acc) { acc.assign(1, 0); }

static int no_engine() { return fail("combine_plans_main: an engine call was reached"); }
int Engine::use() { return no_engine(); }
int Engine::ks_pbs_dev(const uint64_t*, const uint32_t*, uint64_t*, uint32_t, bool) { return no_engine(); }
int Engine::lincomb_dev(const uint64_t*, const uint32_t*, const uint32_t*, const int32_t*, const uint64_t*, uint64_t*, uint32_t) { return no_engine(); }
int Engine::restride_dev(const uint64_t*, uint64_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { return no_engine(); }
int Engine::lincomb_batch_dev(const uint64_t*, const uint32_t*, const uint32_t*, const int32_t*, const uint64_t*, uint64_t*, uint32_t, uint32_t,
                              uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t*) { return no_engine(); }
int Engine::lut_upload_dedup(const std::vector<uint64_t>&, uint32_t*) { return no_engine(); }
int MultiCuRuntime::check() { return no_engine(); }
int Pipeline::wait_all(hipStream_t) { return no_engine(); }

int build_string_op(Circuit& c, const std::string& op, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len);

}  // namespace fhe

static size_t built = 0, refused = 0;

// One plan: want_outputs output blocks, or (expect != nullptr) a refusal that names `expect`.  false: not as expected.
static bool one(const fhe_params_t& p, const std::string& name, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len,
                uint32_t want_outputs, const char* expect) {
    for (uint32_t world = 1; world <= 2; world++) {
        fhe::Circuit c(p, nullptr);
        c.set_build_world(world);
        if (fhe::build_string_op(c, name, a_cap, b_cap, clear, clear_len)) {
            std::printf("%s msg_mod=%u a_cap=%u b_cap=%u world=%u\trefused\t%s\n", name.c_str(), p.msg_mod, a_cap, b_cap, world, fhe::g_error.c_str());
            if (!expect || fhe::g_error.find(expect) == std::string::npos) return false;
            refused++;
            continue;
        }
        if (expect || c.finalize(world)) {
            std::printf("%s msg_mod=%u world=%u\tnot as expected\t%s\n", name.c_str(), p.msg_mod, world, fhe::g_error.c_str());
            return false;
        }
        std::printf("%s msg_mod=%u a_cap=%u b_cap=%u world=%u\t%u inputs, %u outputs, %u levels, %u pbs, noise %.1f of %.1f\n", name.c_str(), p.msg_mod,
                    a_cap, b_cap, world, c.n_inputs(), c.n_outputs(), c.n_levels(), c.n_pbs(), c.max_pbs_input_noise(), c.noise_budget());
        if (c.n_outputs() != want_outputs || c.n_pbs() == 0 || c.n_levels() == 0 || c.max_pbs_input_noise() > c.noise_budget()) {
            std::printf("%s\twrong shape: want %u outputs\n", name.c_str(), want_outputs);
            return false;
        }
        built++;
    }
    return true;
}

int main() {
    // {n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg_mod, carry_mod, lwe_std, glwe_std}: 2-bit blocks (four per
    // character, a box of 16) and 4-bit blocks (two per character, a box of 256)
    fhe_params_t sets[2] = {};
    sets[0].n = 16, sets[0].k = 1, sets[0].N = 256, sets[0].pbs_base_log = 10, sets[0].pbs_level = 2, sets[0].ks_base_log = 4, sets[0].ks_level = 4;
    sets[0].msg_mod = sets[0].carry_mod = 4, sets[0].lwe_std = 1e-12, sets[0].glwe_std = 1e-15;
    sets[1].n = 4, sets[1].k = 1, sets[1].N = 32768, sets[1].pbs_base_log = 15, sets[1].pbs_level = 2, sets[1].ks_base_log = 3, sets[1].ks_level = 7;
    sets[1].msg_mod = sets[1].carry_mod = 16, sets[1].lwe_std = 1e-13, sets[1].glwe_std = 1e-17;
    const uint8_t text[] = {'x', 'y'};
    const char* counts[] = {"count_add", "count_sub", "count_eq", "count_ne", "count_lt", "count_le", "count_gt", "count_ge"};
    auto s = [](uint32_t v) { return std::to_string(v); };
    for (const fhe_params_t& p : sets) {
        const uint32_t bpc = fhe::opname::blocks_per_char(p.msg_mod);
        auto digits = [&](uint64_t n_max) { return fhe::opname::count_digits(p.msg_mod, n_max); };
        for (uint32_t k = 1; k <= 9; k++) {
            for (const char* op : {"and", "or", "xor"})
                if (!one(p, std::string(op) + ":" + s(k), 0, 0, nullptr, 0, 1, k < 2 ? "k must be at least 2" : nullptr)) return 1;
            if (!one(p, "not:" + s(k), 0, 0, nullptr, 0, k, nullptr)) return 1;
        }
        for (uint32_t cap = 1; cap <= 9; cap++)
            for (uint32_t out_cap : {1u, cap, cap + 2}) {
                for (uint32_t b_cap : {1u, 9u})
                    if (!one(p, "select:" + s(out_cap), cap, b_cap, nullptr, 0, out_cap * bpc, nullptr)) return 1;
                for (uint32_t len : {0u, 2u})
                    if (!one(p, "select_clear:" + s(out_cap), cap, 0, text, len, out_cap * bpc, nullptr)) return 1;
            }
        for (uint32_t a_max = 1; a_max <= 9; a_max++) {
            for (uint32_t b_max = 1; b_max <= 9; b_max++) {
                if (!one(p, "select_count:" + s(a_max) + ":" + s(b_max), 0, 0, nullptr, 0, digits(std::max(a_max, b_max)), nullptr)) return 1;
                for (const char* op : counts) {
                    const std::string base = op;
                    const uint32_t want = base == "count_add" ? digits(a_max + b_max) : base == "count_sub" ? digits(a_max) : 1;
                    if (!one(p, base + ":" + s(a_max) + ":" + s(b_max), 0, 0, nullptr, 0, want, nullptr)) return 1;
                }
            }
            for (uint32_t k : {0u, 1u, a_max, a_max + 1, 300u})            // the clear integer, in one byte and in two
                for (const char* op : counts) {
                    const std::string base = op;
                    const uint8_t bytes[2] = {(uint8_t)(k & 255), (uint8_t)(k >> 8)};
                    const uint32_t want = base == "count_add" ? digits(a_max + k) : base == "count_sub" ? digits(a_max) : 1;
                    if (!one(p, base + "_clear:" + s(a_max), 0, 0, bytes, k > 255 ? 2 : 1, want, nullptr)) return 1;
                }
        }
        // three-digit counts on either block width: bounds that are multiples of a unit, bounds that are not, a second operand of
        // one unit -- the sums whose clamps run beside the carry chain, and the radix code behind them
        for (uint32_t a_max : {16u, 20u, 32u, 48u, 63u, 256u, 300u, 512u}) {
            for (uint32_t b_max : {5u, 16u, 20u, 63u})
                for (const char* op : counts) {
                    const std::string base = op;
                    const uint32_t want = base == "count_add" ? digits(a_max + b_max) : base == "count_sub" ? digits(a_max) : 1;
                    if (!one(p, base + ":" + s(a_max) + ":" + s(b_max), 0, 0, nullptr, 0, want, nullptr)) return 1;
                }
            for (uint32_t k : {1u, 300u})
                for (const char* op : counts) {
                    const std::string base = op;
                    const uint8_t bytes[2] = {(uint8_t)(k & 255), (uint8_t)(k >> 8)};
                    const uint32_t want = base == "count_add" ? digits(a_max + k) : base == "count_sub" ? digits(a_max) : 1;
                    if (!one(p, base + "_clear:" + s(a_max), 0, 0, bytes, k > 255 ? 2 : 1, want, nullptr)) return 1;
                }
        }
    }
    std::printf("%zu built, %zu refused\n", built, refused);
    return 0;
}
