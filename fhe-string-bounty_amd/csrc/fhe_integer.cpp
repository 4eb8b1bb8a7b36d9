// fhe_integer.cpp -- radix-integer operations of the reference's integer layer as batched shortint
// circuits: the callers on the other side of the apply_lookup_table boundary that
// the string operations lean on, exposed through the plan ABI (fhe_int_plan_create).
//
// An unsigned radix integer = n_blocks shortint blocks, little endian, log2(msg_mod) bits each
// (integer/block_decomposition.rs:119-144).  Restated from the reference:
//   add / sub / scalar_add / scalar_sub   unchecked add, then the one-carry parallel propagation:
//        generate-or-propagate state per block, Hillis-Steele prefix scan of the states, add the incoming
//        carry, message_extract
//        (integer/server_key/radix_parallel/add.rs:13-42,487-542 propagate_single_carry_parallelized_low_latency,
//         :544-624 compute_prefix_sum_hillis_steele, :724-772 generate_init_carry_array;
//         scalar_add.rs:204-222; subtraction as a + (2^bits - 1 - b) + 1, the two's complement the
//         reference reaches through neg.rs's correcting terms)
//   message_extract / carry_extract       shortint/server_key/mod.rs (x % msg_mod, x / msg_mod)
//   cmux (if_then_else)                   radix_parallel/cmux.rs:194-248: zero out each side by the
//        condition (one lookup per block and side), add, message_extract
//   eq / ne / gt / ge / lt / le (+ scalar_*)   integer/server_key/comparator.rs:193-280: pack two blocks,
//        true LWE subtraction whose sign lands in the padding bit, sign lookup + 1 in {0, 1, 2},
//        pairwise reduction 4*msb + lsb, final sign -> bool lookup; equality through
//        radix_parallel/scalar_comparison.rs:147-233.  Block by block where two packed pairs exceed the noise budget
//        (RadixOps::two_pairs_fit); a scalar beyond the integer's range is decided at build (scalar_comparison.rs:23-60)
// Every lookup of one level of one operation is one batched KS+PBS launch (circuit.h).
#include <algorithm>
#include <string>

#include "circuit.h"
#include "radix_ops.h"

namespace fhe {

// op in {add, sub, scalar_add, scalar_sub, message_extract, carry_extract, cmux, eq, ne, gt, ge, lt, le,
// scalar_eq, scalar_ne, scalar_gt, scalar_ge, scalar_lt, scalar_le}.  Inputs, in order: [cond (cmux only)],
// a (n_blocks), [b (n_blocks) for the two-operand forms].  Outputs: n_blocks blocks, or one 0/1 block.
int build_integer_op(Circuit& c, const std::string& op, uint32_t n_blocks, uint64_t scalar) {
    RadixOps r(c);
    if (!r.ok()) return fail("integer ops need msg_mod = 2^b >= 2 and carry_mod >= msg_mod");
    if (n_blocks == 0) return fail("n_blocks must be > 0");
    if ((uint64_t)n_blocks * r.bits > 64 && op.compare(0, 7, "scalar_") == 0) return fail("scalar operands are limited to 64 bits");
    auto emit = [&](const std::vector<uint32_t>& v) { for (uint32_t b : v) c.output(b); };
    const bool is_scalar = op.compare(0, 7, "scalar_") == 0;
    const std::string base = is_scalar ? op.substr(7) : op;
    // two encrypted operands: compare block by block where two packed pairs exceed the budget (scalar forms pack one pair)
    if (!is_scalar) r.pair_blocks = r.two_pairs_fit();
    // is_scalar_out_of_bounds (radix_parallel/scalar_comparison.rs:23-60): a scalar with bits beyond the integer's is
    // above every value of it, and the answer is known here.  scalar_add / scalar_sub wrap instead.  The plan keeps
    // its inputs; its output is a constant table read on the first of them, a lookup's result like every other output.
    const uint32_t total_bits = n_blocks * r.bits;
    const bool above = is_scalar && total_bits < 64 && (scalar >> total_bits) != 0;
    if (above && base != "add" && base != "sub") {
        const bool known = base == "ne" || base == "lt" || base == "le";
        if (!known && base != "eq" && base != "gt" && base != "ge") return fail("unknown integer op: " + op);
        const auto a = r.input(n_blocks);
        c.output(c.pbs(a[0], c.lut_fn([known](uint64_t) { return (uint64_t)known; })));
        if (c.failed()) return fail("circuit build error: " + c.error());
        return 0;
    }
    if (op == "cmux") {
        const uint32_t cond = c.input(1);
        const auto t = r.input(n_blocks), f = r.input(n_blocks);
        emit(r.cmux(cond, t, f));
    } else if (op == "message_extract" || op == "carry_extract") {
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < n_blocks; i++) v.push_back(c.input(r.T - 1));   // blocks with full carries
        for (uint32_t b : v) c.output(op == "message_extract" ? r.message_extract(b) : r.carry_extract(b));
    } else if (base == "add" || base == "sub") {
        const auto a = r.input(n_blocks);
        if (is_scalar) emit(base == "add" ? r.scalar_add(a, scalar) : r.scalar_sub(a, scalar));
        else { const auto b = r.input(n_blocks); emit(base == "add" ? r.add(a, b) : r.sub(a, b)); }
    } else if (base == "eq" || base == "ne") {
        const auto a = r.input(n_blocks);
        if (is_scalar) c.output(r.eq(a, nullptr, scalar, base == "eq"));
        else { const auto b = r.input(n_blocks); c.output(r.eq(a, &b, 0, base == "eq")); }
    } else if (base == "gt" || base == "ge" || base == "lt" || base == "le") {
        const auto a = r.input(n_blocks);
        uint32_t s;
        if (is_scalar) s = r.sign(a, nullptr, scalar);
        else { const auto b = r.input(n_blocks); s = r.sign(a, &b, 0); }
        const bool lt = base == "lt", le = base == "le", gt = base == "gt";
        c.output(c.pbs(s, c.lut_fn([lt, le, gt](uint64_t x) { return (uint64_t)(lt ? x == 0 : (le ? x != 2 : (gt ? x == 2 : x != 0))); })));
    } else {
        return fail("unknown integer op: " + op);
    }
    if (c.failed()) return fail("circuit build error: " + c.error());
    return 0;
}

}  // namespace fhe
