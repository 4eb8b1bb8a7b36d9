// integer_plans_main.cpp -- the planner units behind the integer plans (csrc/circuit.cpp, fhe_integer.cpp; radix_ops.h is a
// header) linked into a stand-alone program that builds every name of build_integer_op offline at block counts 1 .. 9, 16
// and 33 on blocks of 1, 2, 3 and 4 bits, and finalises each plan for one and for two ranks.  It prints one line per plan:
// its info, or the refusal.  Compiled under the host sanitizers by tests/test_integer_host.py; nothing is loaded into Python
// and no device is touched: a circuit without an engine never reaches the engine's device calls, which are stubs below, and
// the tables' accumulators -- read only when a plan runs -- are left empty.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "circuit.h"

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

static int no_engine() { return fail("integer_plans_main: an engine call was reached"); }
int Engine::use() { return no_engine(); }
int Engine::ks_pbs_dev(const uint64_t*, const uint32_t*, uint64_t*, uint32_t, bool) { return no_engine(); }
int Engine::lincomb_dev(const uint64_t*, const uint32_t*, const uint32_t*, const int32_t*, const uint64_t*, uint64_t*, uint32_t) { return no_engine(); }
int Engine::restride_dev(const uint64_t*, uint64_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { return no_engine(); }
int Engine::lincomb_batch_dev(const uint64_t*, const uint32_t*, const uint32_t*, const int32_t*, const uint64_t*, uint64_t*, uint32_t, uint32_t,
                              uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t*) { return no_engine(); }
int Engine::lut_upload_dedup(const std::vector<uint64_t>&, uint32_t*) { return no_engine(); }
int MultiCuRuntime::check() { return no_engine(); }
int Pipeline::wait_all(hipStream_t) { return no_engine(); }

int build_integer_op(Circuit& c, const std::string& op, uint32_t n_blocks, uint64_t scalar);

}  // namespace fhe

static size_t built = 0, refused = 0;

// One plan in both worlds: want_outputs output blocks, or (expect != nullptr) a refusal that names `expect`.  false: not as expected.
static bool one(const fhe_params_t& p, const std::string& name, uint32_t n, uint64_t scalar, uint32_t want_inputs, uint32_t want_outputs,
                const char* expect) {
    for (uint32_t world = 1; world <= 2; world++) {
        fhe::Circuit c(p, nullptr);
        c.set_build_world(world);
        if (fhe::build_integer_op(c, name, n, scalar)) {
            std::printf("%s msg_mod=%u box=%u blocks=%u world=%u\trefused\t%s\n", name.c_str(), p.msg_mod, p.msg_mod * p.carry_mod, n, world,
                        fhe::g_error.c_str());
            if (!expect || fhe::g_error.find(expect) == std::string::npos) return false;
            refused++;
            continue;
        }
        if (expect || c.finalize(world)) {
            std::printf("%s msg_mod=%u blocks=%u world=%u\tnot as expected\t%s\n", name.c_str(), p.msg_mod, n, world, fhe::g_error.c_str());
            return false;
        }
        std::printf("%s msg_mod=%u box=%u blocks=%u world=%u\t%u inputs, %u outputs, %u levels, %u pbs, noise %.1f of %.1f\n", name.c_str(), p.msg_mod,
                    p.msg_mod * p.carry_mod, n, world, c.n_inputs(), c.n_outputs(), c.n_levels(), c.n_pbs(), c.max_pbs_input_noise(), c.noise_budget());
        if (c.n_inputs() != want_inputs || c.n_outputs() != want_outputs || c.n_pbs() == 0 || c.n_levels() == 0 ||
            c.max_pbs_input_noise() > c.noise_budget()) {
            std::printf("%s\twrong shape: want %u inputs, %u outputs\n", name.c_str(), want_inputs, want_outputs);
            return false;
        }
        built++;
    }
    return true;
}

int main() {
    // {n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg_mod, carry_mod, lwe_std, glwe_std}: blocks of 1 bit in a
    // box of 32 and in a box of 8 (which cannot hold two scan states), of 2 bits in a box of 16, of 3 in 64, of 4 in 256
    struct Set { uint32_t n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg_mod, carry_mod; double lwe_std, glwe_std; };
    const Set shapes[5] = {{6, 1, 4096, 15, 2, 3, 6, 2, 16, 1e-13, 1e-17}, {6, 1, 4096, 15, 2, 3, 6, 2, 4, 1e-13, 1e-17},
                           {16, 1, 256, 10, 2, 4, 4, 4, 4, 1e-12, 1e-15},  {8, 1, 8192, 15, 2, 3, 6, 8, 8, 1e-13, 1e-17},
                           {4, 1, 32768, 15, 2, 3, 7, 16, 16, 1e-13, 1e-17}};
    const char* two[] = {"add", "sub", "eq", "ne", "gt", "ge", "lt", "le"};
    for (const Set& s : shapes) {
        fhe_params_t p = {};
        p.n = s.n, p.k = s.k, p.N = s.N, p.pbs_base_log = s.pbs_base_log, p.pbs_level = s.pbs_level, p.ks_base_log = s.ks_base_log;
        p.ks_level = s.ks_level, p.msg_mod = s.msg_mod, p.carry_mod = s.carry_mod, p.lwe_std = s.lwe_std, p.glwe_std = s.glwe_std;
        uint32_t bits = 0;
        while ((1u << bits) < p.msg_mod) bits++;
        const bool small_box = p.msg_mod == 2 && p.msg_mod * p.carry_mod < 11;
        for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 16u, 33u}) {
            const char* no_scan = small_box && n >= 3 ? "beyond the box" : nullptr;
            const char* no_signs = small_box && n >= 3 ? "input degree 10 overflows" : nullptr;
            for (const char* op : two) {
                const std::string base = op;
                const bool sum = base == "add" || base == "sub", order = base[0] == 'g' || base[0] == 'l';
                if (!one(p, base, n, 0, 2 * n, sum ? n : 1, sum ? no_scan : order ? no_signs : nullptr)) return 1;
                // 5 is beyond the range of one block of 1 or 2 bits: those comparisons are decided at build
                const char* expect = n * bits > 64 ? "limited to 64 bits" : sum ? no_scan : order ? no_signs : nullptr;
                if (!one(p, "scalar_" + base, n, 5, n, sum ? n : 1, expect)) return 1;
            }
            if (!one(p, "message_extract", n, 0, n, n, nullptr) || !one(p, "carry_extract", n, 0, n, n, nullptr)) return 1;
            if (!one(p, "cmux", n, 0, 2 * n + 1, n, nullptr)) return 1;
        }
        if (!one(p, "mul", 4, 0, 0, 0, "unknown integer op") || !one(p, "scalar_mul", 1, 5, 0, 0, "unknown integer op")) return 1;
    }
    std::printf("%zu built, %zu refused\n", built, refused);
    return 0;
}
