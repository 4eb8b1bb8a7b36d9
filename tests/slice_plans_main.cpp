// slice_plans_main.cpp -- the planner units (csrc/circuit.cpp, fhe_string.cpp, the str_*.cpp units behind str_ops.h with
// str_slice.cpp among them, regex.cpp, str_op_name.cpp) linked into a stand-alone program that builds every name of the
// slice family offline at capacities 1 .. 9, on 2-bit and on 4-bit blocks, and finalises each plan for one and for two
// ranks.  Compiled under the host sanitizers by tests/test_slice_host.py; nothing is loaded into Python and no device is
// touched: a circuit without an engine never reaches the engine's device calls, which are stubs below, and the tables'
// accumulators -- read only when a plan runs -- are left empty.
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

static int no_engine() { return fail("slice_plans_main: an engine call was reached"); }
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

int main() {
    // {n, k, N, pbs_base_log, pbs_level, ks_base_log, ks_level, msg_mod, carry_mod, lwe_std, glwe_std}: 2-bit blocks (four per
    // character, a box of 16) and 4-bit blocks (two per character, a box of 256)
    fhe_params_t sets[2] = {};
    sets[0].n = 16, sets[0].k = 1, sets[0].N = 256, sets[0].pbs_base_log = 10, sets[0].pbs_level = 2, sets[0].ks_base_log = 4, sets[0].ks_level = 4;
    sets[0].msg_mod = sets[0].carry_mod = 4, sets[0].lwe_std = 1e-12, sets[0].glwe_std = 1e-15;
    sets[1].n = 4, sets[1].k = 1, sets[1].N = 32768, sets[1].pbs_base_log = 15, sets[1].pbs_level = 2, sets[1].ks_base_log = 3, sets[1].ks_level = 7;
    sets[1].msg_mod = sets[1].carry_mod = 16, sets[1].lwe_std = 1e-13, sets[1].glwe_std = 1e-17;
    const char* bases[] = {"take", "skip", "split_at", "char_at", "insert"};
    const uint8_t text[] = {'x', 'y'};
    size_t built = 0, refused = 0;
    for (const fhe_params_t& p : sets)
        for (uint32_t a_cap = 1; a_cap <= 9; a_cap++)
            for (const char* base : bases)
                for (int enc = 0; enc < 2; enc++)
                    for (int form = 0; form < (std::string(base) == "insert" ? 3 : 1); form++)       // t: encrypted, clear, clear and empty
                        for (uint32_t at : {0u, 1u, a_cap - 1, a_cap, a_cap + 1, 2 * a_cap + 3})
                            for (uint32_t out_cap : {0u, 1u, a_cap + 2})
                                for (uint32_t world = 1; world <= 2; world++) {
                                    const bool inserts = std::string(base) == "insert", one_char = std::string(base) == "char_at";
                                    if (one_char && out_cap) continue;
                                    std::string name = std::string(base) + (enc ? "_encn" : "") + (inserts && form ? "_clear" : "") + ":" + std::to_string(at);
                                    if (out_cap) name += ":" + std::to_string(out_cap);
                                    fhe::Circuit c(p, nullptr);
                                    c.set_build_world(world);
                                    const int rc = fhe::build_string_op(c, name, a_cap, inserts && !form ? 2 : 0, form ? text : nullptr, form == 1 ? 2 : 0);
                                    const bool expect_refusal = enc && at == 0;                       // n_max = 0
                                    if (rc) {
                                        refused++;
                                        if (!expect_refusal || fhe::g_error.find("n_max must be at least 1") == std::string::npos) {
                                            std::printf("%s msg_mod=%u a_cap=%u world=%u\trefused\t%s\n", name.c_str(), p.msg_mod, a_cap, world, fhe::g_error.c_str());
                                            return 1;
                                        }
                                        continue;
                                    }
                                    if (expect_refusal || c.finalize(world)) {
                                        std::printf("%s msg_mod=%u a_cap=%u world=%u\tnot as expected\t%s\n", name.c_str(), p.msg_mod, a_cap, world, fhe::g_error.c_str());
                                        return 1;
                                    }
                                    const uint32_t bpc = fhe::opname::blocks_per_char(p.msg_mod);
                                    const uint32_t cap = out_cap ? out_cap : a_cap + (inserts ? (form == 0 ? 2 : form == 1 ? 2 : 0) : 0);
                                    const uint32_t want = one_char ? 1 + bpc : (std::string(base) == "split_at" ? 2 : 1) * cap * bpc;
                                    if (c.n_outputs() != want || c.n_pbs() == 0 || c.max_pbs_input_noise() > c.noise_budget()) {
                                        std::printf("%s msg_mod=%u a_cap=%u world=%u\twrong shape\t%u outputs (want %u), %u pbs, noise %.1f\n", name.c_str(),
                                                    p.msg_mod, a_cap, world, c.n_outputs(), want, c.n_pbs(), c.max_pbs_input_noise());
                                        return 1;
                                    }
                                    built++;
                                }
    std::printf("%zu built, %zu refused\n", built, refused);
    return 0;
}
