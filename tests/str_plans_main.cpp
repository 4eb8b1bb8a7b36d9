// str_plans_main.cpp -- builds FheString plans offline through the C ABI, one plan key per line of standard input, and
// prints each plan's info or its refusal.  A stand-alone program, so that the plan builder (csrc/fhe_string.cpp and the
// str_*.cpp units behind str_ops.h) runs under the host sanitizers without Python: `make sanitize-plans` in
// fhe-string-bounty_amd/.  No GPU is touched: the plans are built from parameters alone.
//
// A key (scripts/plan_digest.py --keys): the fields of fhe_params_t in declaration order, world, plan name, a_cap, b_cap,
// and the clear bytes as `x` + hex digits (`-`: no clear operand).
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fhestr.h"

int main() {
    std::string line;
    size_t built = 0, refused = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        fhe_params_t p{};
        uint32_t world = 0, a_cap = 0, b_cap = 0;
        std::string name, hex;
        in >> p.n >> p.k >> p.N >> p.pbs_base_log >> p.pbs_level >> p.ks_base_log >> p.ks_level >> p.msg_mod >> p.carry_mod >>
            p.lwe_std >> p.glwe_std >> p.grouping_factor >> world >> name >> a_cap >> b_cap >> hex;
        if (!in || (hex != "-" && (hex[0] != 'x' || hex.size() % 2 == 0))) {
            std::fprintf(stderr, "bad key: %s\n", line.c_str());
            return 2;
        }
        std::vector<uint8_t> clear;
        for (size_t i = 1; i + 1 < hex.size(); i += 2) clear.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
        const uint8_t* bytes = hex == "-" ? nullptr : clear.data();
        std::printf("N=%u msg=%u world=%u %s %u %u %s: ", p.N, p.msg_mod, world, name.c_str(), a_cap, b_cap, hex.c_str());
        fhe_plan* plan = nullptr;
        if (fhe_str_plan_create_offline(&p, name.c_str(), a_cap, b_cap, bytes, (uint32_t)clear.size(), world, &plan)) {
            std::printf("refused: %s\n", fhe_last_error());
            refused++;
            continue;
        }
        uint32_t info[6] = {0, 0, 0, 0, 0, 0};
        if (fhe_plan_info(plan, info)) {
            std::fprintf(stderr, "fhe_plan_info: %s\n", fhe_last_error());
            return 1;
        }
        std::printf("%u %u %u %u %u %u\n", info[0], info[1], info[2], info[3], info[4], info[5]);
        fhe_plan_destroy(plan);
        built++;
    }
    std::printf("%zu keys: %zu built, %zu refused\n", built + refused, built, refused);
    return 0;
}
