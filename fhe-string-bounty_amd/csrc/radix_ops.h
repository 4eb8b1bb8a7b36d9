// radix_ops.h -- RadixOps: the radix-integer building blocks of the reference's integer layer as batched shortint
// circuits: add and subtract with the one-carry parallel propagation, the comparator, equality, cmux.  Shared by the
// integer plans (fhe_integer.cpp, which names the reference's sources) and the count arithmetic of the FheString plans
// (count_ops.h).  An unsigned radix integer = n blocks, little endian, log2(msg_mod) bits each.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "circuit.h"

namespace fhe {

struct RadixOps {
    Circuit& c;
    uint32_t M, T, bits;
    explicit RadixOps(Circuit& c) : c(c), M(c.msg_modulus()), T(c.total_modulus()), bits(0) {
        while ((1u << bits) < M) bits++;
    }
    bool ok() const { return (1u << bits) == M && M >= 2 && T / M >= M; }

    std::vector<uint32_t> input(uint32_t n) {
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < n; i++) v.push_back(c.input(M - 1));
        return v;
    }
    std::vector<uint32_t> digits(uint64_t x, uint32_t n) const {
        std::vector<uint32_t> d;
        for (uint32_t i = 0; i < n; i++) { d.push_back((uint32_t)(x & (M - 1))); x >>= bits; }
        return d;
    }
    uint32_t message_extract(uint32_t b) { const uint32_t m = M; return c.pbs(b, c.lut_fn([m](uint64_t x) { return x % m; })); }
    uint32_t carry_extract(uint32_t b) { const uint32_t m = M; return c.pbs(b, c.lut_fn([m](uint64_t x) { return x / m; })); }

    // An answer known beforehand for one case: where the 0/1 block `flag` is set, output block i is digits[i] whatever the
    // sums hold.  The flag rides on the last lookup of every block, next to the sum (2M * flag: needs 4M <= T), so it
    // is computed beside the carry chain and costs no level.
    struct Late {
        uint32_t flag;
        std::vector<uint64_t> digits;
    };
    bool late_fits(uint32_t flag, double budget) const { return 4 * M <= T && 2.0 + 4.0 * M * M * c.node(flag).noise <= budget; }
    // propagate_single_carry_parallelized_low_latency (add.rs:518-542): sums[i] in [0, 2M-1]
    // carry_out: one more block, the carry out of the last one (a sum that needs one digit more than its operands)
    //
    // Two scan states share one lookup input as base * later + earlier.  A state has three values, so the base is M only
    // from M = 4 on; 1-bit blocks take base 4, which a box below 4 * 2 + 2 + 1 = 11 cannot hold: refused.  The state of
    // the last block is never read; 1-bit blocks do not scan it (wider blocks do, as their plans always have), so two
    // blocks need no scan and build in any box.
    uint32_t scan_base() const { return std::max(M, 4u); }
    std::vector<uint32_t> propagate(const std::vector<uint32_t>& sums, bool carry_out = false, const Late* late = nullptr) {
        const uint32_t n = (uint32_t)sums.size(), m = M, base = scan_base();
        const uint32_t scanned = m >= 4 ? n : n - 1;
        if (scanned > 1 && base != m && 2 * base + 2 >= T) {
            c.refuse("carry propagation over " + std::to_string(n) + " blocks: msg_mod " + std::to_string(m) + " packs two scan states in base " +
                     std::to_string(base) + ", up to " + std::to_string(2 * base + 2) + ", beyond the box msg_mod * carry_mod = " + std::to_string(T));
            return std::vector<uint32_t>(n + (carry_out ? 1 : 0), c.trivial(0));
        }
        // generate_init_carry_array (add.rs:724-772): 0 = None, 1 = Generated, 2 = Propagated
        const uint32_t first = c.lut_fn([m](uint64_t x) { return (uint64_t)(x >= m ? 1 : 0); });
        const uint32_t other = c.lut_fn([m](uint64_t x) { return (uint64_t)(x >= m ? 1 : (x == m - 1 ? 2 : 0)); });
        std::vector<uint32_t> st(n);
        for (uint32_t i = 0; i < n; i++) st[i] = c.pbs(sums[i], i == 0 ? first : other);
        // compute_prefix_sum_hillis_steele (add.rs:572-624) with prefix_sum_carry_propagation (add.rs:36-42)
        const uint32_t comb = c.lut_fn([base](uint64_t x) { const uint64_t msb = (x / base) % base, lsb = x % base; return msb == 2 ? lsb : msb; });
        for (uint32_t space = 1; space < scanned; space *= 2) {
            std::vector<uint32_t> next(st);
            for (uint32_t i = space; i < scanned; i++) next[i] = c.pbs(c.lin({{st[i], (int32_t)base}, {st[i - space], 1}}), comb);
            st.swap(next);
        }
        // the output carry of block i-1 is the input carry of block i; add, then message_extract
        auto last = [&](uint32_t value, size_t block, bool carry) {
            if (!late) return carry ? carry_extract(value) : message_extract(value);
            const uint64_t known = late->digits[block], two = 2 * m;
            // (a sum with its carry is at most 2M - 1, whatever interval arithmetic makes of the scanned states)
            return c.pbs(c.lin({{value, 1}, {late->flag, (int32_t)two}}, 0, (int64_t)(2 * two - 1)),
                         c.lut_fn([=](uint64_t x) { return x >= two ? known : carry ? x / m : x % m; }));
        };
        std::vector<uint32_t> out(n);
        for (uint32_t i = 0; i < n; i++)
            out[i] = last(i == 0 ? sums[0] : c.lin({{sums[i], 1}, {st[i - 1], 1}}), i, false);
        if (carry_out) out.push_back(last(n == 1 ? sums[0] : c.lin({{sums[n - 1], 1}, {st[n - 2], 1}}), n, true));
        return out;
    }
    std::vector<uint32_t> add(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, bool carry_out = false) {
        std::vector<uint32_t> s;
        for (size_t i = 0; i < a.size(); i++) s.push_back(c.lin({{a[i], 1}, {b[i], 1}}));   // unchecked_add (add.rs:88-100)
        return propagate(s, carry_out);
    }
    std::vector<uint32_t> sub(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
        std::vector<uint32_t> s;   // a + (2^bits - 1 - b) + 1
        for (size_t i = 0; i < a.size(); i++) s.push_back(c.lin({{a[i], 1}, {b[i], -1}}, (int64_t)M - 1 + (i == 0 ? 1 : 0)));
        return propagate(s);
    }
    std::vector<uint32_t> scalar_add(const std::vector<uint32_t>& a, uint64_t scalar, bool carry_out = false, const Late* late = nullptr) {
        const auto d = digits(scalar, (uint32_t)a.size());
        std::vector<uint32_t> s;
        for (size_t i = 0; i < a.size(); i++) s.push_back(c.lin({{a[i], 1}}, d[i]));       // unchecked_scalar_add (scalar_add.rs)
        return propagate(s, carry_out, late);
    }
    std::vector<uint32_t> scalar_sub(const std::vector<uint32_t>& a, uint64_t scalar) {
        const uint32_t total_bits = bits * (uint32_t)a.size();
        const uint64_t mask = total_bits >= 64 ? ~0ull : ((1ull << total_bits) - 1);
        return scalar_add(a, (0 - scalar) & mask);
    }
    // zero_out_if + add + message_extract (cmux.rs:194-316)
    std::vector<uint32_t> cmux(uint32_t cond, const std::vector<uint32_t>& t, const std::vector<uint32_t>& f) {
        const uint32_t m2 = 2 * M;
        const uint32_t keep_set = c.lut_fn([m2](uint64_t x) { return (uint64_t)((x < m2 && (x & 1)) ? x >> 1 : 0); });
        const uint32_t keep_clear = c.lut_fn([m2](uint64_t x) { return (uint64_t)((x < m2 && !(x & 1)) ? x >> 1 : 0); });
        std::vector<uint32_t> out;
        for (size_t i = 0; i < t.size(); i++) {
            const uint32_t a = c.pbs(c.lin({{cond, 1}, {t[i], 2}}), keep_set);
            const uint32_t b = c.pbs(c.lin({{cond, 1}, {f[i], 2}}), keep_clear);
            out.push_back(message_extract(c.lin({{a, 1}, {b, 1}}, 0, M - 1)));
        }
        return out;
    }
    // are_all_comparisons_block_true / is_at_least_one (scalar_comparison.rs:147-233)
    uint32_t reduce(std::vector<uint32_t> bits_, bool all) {
        if (bits_.empty()) return c.trivial(all ? 1 : 0);
        const uint32_t nz = c.lut_fn([](uint64_t x) { return (uint64_t)(x != 0); });
        while (bits_.size() > 1) {
            std::vector<uint32_t> next;
            for (size_t i = 0; i < bits_.size(); i += T - 1) {
                const size_t len = std::min<size_t>(T - 1, bits_.size() - i);
                std::vector<Term> terms;
                for (size_t j = 0; j < len; j++) terms.push_back({bits_[i + j], 1});
                next.push_back(c.pbs(c.lin(terms), all ? c.lut_fn([len](uint64_t x) { return (uint64_t)(x == len); }) : nz));
            }
            bits_.swap(next);
        }
        return bits_[0];
    }
    // packed pairs hi*M + lo as LIN nodes (pack_block_chunk, scalar_comparison.rs:104-138); a trailing
    // single block stays alone.  Encrypted operand or clear digits.
    bool pair_blocks = true;       // false: every block is compared on its own (where two packed operands exceed the noise budget)
    // the comparator subtracts two packed pairs: 2 (1 + M^2) variances, beyond the budget of 4-bit blocks
    bool two_pairs_fit() const {
        const double budget = c.noise_budget() > 0 ? c.noise_budget() : 1e300;
        return (uint64_t)M * M <= (uint64_t)T && 2.0 * (1.0 + (double)M * M) <= budget;
    }
    std::vector<uint32_t> packed(const std::vector<uint32_t>& a) {
        if (!pair_blocks) return a;
        std::vector<uint32_t> p;
        for (size_t i = 0; i < a.size(); i += 2)
            p.push_back(i + 1 < a.size() ? c.lin({{a[i], 1}, {a[i + 1], (int32_t)M}}) : a[i]);
        return p;
    }
    std::vector<uint32_t> packed_clear(const std::vector<uint32_t>& d) const {
        if (!pair_blocks) return d;
        std::vector<uint32_t> p;
        for (size_t i = 0; i < d.size(); i += 2) p.push_back(i + 1 < d.size() ? d[i] + d[i + 1] * M : d[i]);
        return p;
    }
    uint32_t eq(const std::vector<uint32_t>& a, const std::vector<uint32_t>* b, uint64_t scalar, bool want_equal) {
        const auto pa = packed(a);
        const uint32_t z = c.lut_fn([](uint64_t x) { return (uint64_t)(x == 0); });
        std::vector<uint32_t> bits_;
        if (b) {
            const auto pb = packed(*b);   // true subtraction: zero iff equal; the sign may reach the padding bit
            for (size_t i = 0; i < pa.size(); i++) bits_.push_back(c.pbs(c.lin({{pa[i], 1}, {pb[i], -1}}), z, true));
        } else {
            const auto pd = packed_clear(digits(scalar, (uint32_t)a.size()));
            for (size_t i = 0; i < pa.size(); i++) {
                const uint32_t v = pd[i];
                bits_.push_back(c.pbs(pa[i], c.lut_fn([v](uint64_t x) { return (uint64_t)(x == v); })));
            }
        }
        const uint32_t all = reduce(bits_, true);
        return want_equal ? all : c.lin({{all, -1}}, 1, 1);
    }
    // comparator.rs:193-280: sign of (a - b) per packed pair, most significant pair wins
    uint32_t sign(const std::vector<uint32_t>& a, const std::vector<uint32_t>* b, uint64_t scalar) {
        const auto pa = packed(a);
        const uint32_t sgn = c.lut_fn([](uint64_t x) { return (uint64_t)(x != 0); });   // odd function: -1 below zero for free
        std::vector<uint32_t> signs;   // least significant first, values {0: <, 1: ==, 2: >}
        if (b) {
            const auto pb = packed(*b);
            for (size_t i = 0; i < pa.size(); i++)
                signs.push_back(c.lin({{c.pbs(c.lin({{pa[i], 1}, {pb[i], -1}}), sgn, true), 1}}, 1, 2));
        } else {
            const auto pd = packed_clear(digits(scalar, (uint32_t)a.size()));
            for (size_t i = 0; i < pa.size(); i++)   // scalar_compare_block_assign (comparator.rs:240-255)
                signs.push_back(c.lin({{c.pbs(c.lin({{pa[i], 1}}, -(int64_t)pd[i]), sgn, true), 1}}, 1, 2));
        }
        // reduce_two_sign_blocks_assign (comparator.rs:257-268): 4 * msb + lsb
        const uint32_t pick = c.lut_fn([](uint64_t x) { const uint64_t msb = (x / 4) & 3, lsb = x & 3; return msb == 1 ? lsb : msb; });
        while (signs.size() > 1) {
            std::vector<uint32_t> next;
            for (size_t i = 0; i + 1 < signs.size(); i += 2) next.push_back(c.pbs(c.lin({{signs[i + 1], 4}, {signs[i], 1}}), pick));
            if (signs.size() & 1) next.push_back(signs.back());
            signs.swap(next);
        }
        return signs[0];
    }
};

}  // namespace fhe
