// count_ops.h -- CountOps: arithmetic and comparisons on encrypted counts ("Combining results").
//
// A count is D little-endian base-M digits with a public bound n_max, D the smallest with M^D > n_max (str_ops.h:
// count_inputs).  An operand above its bound acts as the bound, as in every _encn name: the operations work on
// a' = min(a, a_max) and b' = min(b, b_max).  Results are digits a lookup returned: each in [0, M - 1], as many as the
// result's bound needs, so they are the count operand of any _encn name as they are.
//
// Small counts never reach the radix code: a count of one or two digits is ONE lookup input (the packed unit hi * M + lo
// of count_thermometer), so
//   - with a clear second operand every result digit is one lookup on the unit, the clamp inside the table: one level;
//   - two single digits are one bivariate lookup input a + M b: one level;
//   - two units whose bounds add up to less than the box: each is clamped to ONE block holding the whole value (a digit
//     that fills its bound is that block already), and the result is read off a' + b' resp. a' - b' + b_max: two levels.
// Everything else is the integer layer's radix arithmetic (radix_ops.h, shared with fhe_integer.cpp): carry propagation,
// the comparator, equality.  Where it can, the clamp runs beside the carry chain and costs no level: with a clear second
// operand [a >= a_max] rides on the last lookup of every block of the sum (build_clear()); with two encrypted operands, the
// longer of three digits, whose three-digit bounds are multiples of M^2 or fill their digits, the flags only gate the
// carries (sum_low_zero()).  Otherwise two encrypted operands whose digits can hold more than their bound are clamped
// first (clamped()).  A sum that needs a digit more than its operands takes it from the last carry, at no level more.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "radix_ops.h"
#include "str_ops.h"

namespace fhe {

struct CountOps {
    Circuit& c;
    StrOps& s;
    RadixOps r;
    using How = opname::How;
    CountOps(Circuit& c, StrOps& s) : c(c), s(s), r(c) { r.pair_blocks = r.two_pairs_fit(); }

    static bool is_bit(How how) { return how != opname::C_ADD && how != opname::C_SUB; }
    // the clear-text definition on clamped operands
    static uint64_t eval(How how, uint64_t a, uint64_t b) {
        switch (how) {
        case opname::C_ADD: return a + b;
        case opname::C_SUB: return a > b ? a - b : 0;
        case opname::C_EQ: return a == b;
        case opname::C_NE: return a != b;
        case opname::C_LT: return a < b;
        case opname::C_LE: return a <= b;
        case opname::C_GT: return a > b;
        default: return a >= b;
        }
    }
    bool pack() const { return (uint64_t)s.M * s.M <= (uint64_t)s.T && 1.0 + (double)s.M * s.M <= s.budget(); }
    bool one_unit(const std::vector<uint32_t>& digits) const { return digits.size() <= (pack() ? 2u : 1u); }
    uint32_t unit(const std::vector<uint32_t>& digits) { return digits.size() == 2 ? c.lin({{digits[0], 1}, {digits[1], (int32_t)s.M}}) : digits[0]; }
    uint64_t holds(const std::vector<uint32_t>& digits) const {                      // the largest value the digits hold
        uint64_t span = 1;
        for (size_t d = 0; d < digits.size() && span <= (1ull << 40); d++) span *= s.M;
        return span - 1;
    }
    // min(n, bound) as ONE block (a count of one unit, bound < T)
    uint32_t whole(const std::vector<uint32_t>& digits, uint32_t bound) {
        if (digits.size() == 1 && holds(digits) <= bound) return digits[0];
        return c.pbs(unit(digits), c.lut_fn([bound](uint64_t x) { return std::min<uint64_t>(x, bound); }));
    }
    // The digits of min(n, bound); digits that cannot hold more than the bound are returned as they are.  One unit: every
    // digit is one lookup on it.  Two units (hi, lo): [lo >= the bound's] and the high unit's order against the bound's in
    // {0, 1, 2} add up to 2 and more exactly where n >= bound, and every digit is one lookup on itself next to that sum.
    // More units: [n >= bound] from count_thermometer, then one lookup per digit.
    std::vector<uint32_t> clamped(const std::vector<uint32_t>& digits, uint32_t bound) {
        if (holds(digits) <= bound) return digits;
        const uint32_t mm = s.M, bits = s.bits_per_block;
        auto of_bound = [=](size_t d) { return (uint64_t)(bound >> (d * bits)) & (mm - 1); };
        std::vector<uint32_t> out;
        if (one_unit(digits)) {
            const uint32_t x = unit(digits);
            for (size_t d = 0; d < digits.size(); d++)
                out.push_back(c.pbs(x, c.lut_fn([=](uint64_t v) { return (std::min<uint64_t>(v, bound) >> (d * bits)) & (mm - 1); })));
            return out;
        }
        uint32_t flag, from;                   // n >= bound  iff  flag >= from
        if (pack() && digits.size() <= 4 && 4 * s.M <= s.T && 1.0 + 2.0 * s.M * s.M <= s.budget()) {
            const uint64_t unit_mod = (uint64_t)s.M * s.M, lo = bound % unit_mod, hi = bound / unit_mod;
            const uint32_t at_least = c.pbs(unit({digits[0], digits[1]}), c.lut_fn([lo](uint64_t v) { return (uint64_t)(v >= lo); }));
            const uint32_t order = c.pbs(unit(std::vector<uint32_t>(digits.begin() + 2, digits.end())),
                                         c.lut_fn([hi](uint64_t v) { return (uint64_t)(v < hi ? 0 : v == hi ? 1 : 2); }));
            flag = c.lin({{at_least, 1}, {order, 1}}), from = 2;
        } else {
            flag = s.count_thermometer(digits, bound, bound)[0], from = 1;
        }
        for (size_t d = 0; d < digits.size(); d++) {
            const uint64_t b = of_bound(d);
            out.push_back(c.pbs(c.lin({{digits[d], 1}, {flag, (int32_t)s.M}}), c.lut_fn([=](uint64_t v) { return v / mm >= from ? b : v % mm; })));
        }
        return out;
    }
    std::vector<uint32_t> padded(std::vector<uint32_t> digits, size_t n) {
        while (digits.size() < n) digits.push_back(c.trivial(0));
        digits.resize(n);
        return digits;
    }
    std::vector<uint32_t> known(uint64_t value, uint32_t n_out, bool bit) {
        std::vector<uint32_t> out;
        for (uint32_t d = 0; d < n_out; d++) out.push_back(c.trivial((int64_t)(bit ? value : (value >> (d * s.bits_per_block)) & (s.M - 1))));
        return out;
    }

    // `how` on a (bound a_max) and b (bound b_max; null: the clear integer `scalar`); n_out result blocks: the digits of a
    // count, or the one bit of a comparison
    std::vector<uint32_t> build(How how, const std::vector<uint32_t>& a, uint32_t a_max, const std::vector<uint32_t>* b, uint32_t b_max,
                                uint64_t scalar, uint32_t n_out) {
        const bool bit = is_bit(how);
        const uint32_t bits = s.bits_per_block, low = s.M - 1, mm = s.M;
        auto part = [bit, bits, low](uint64_t value, uint32_t d) { return bit ? value : (value >> (d * bits)) & low; };
        std::vector<uint32_t> out;
        if (!b && one_unit(a)) {
            const uint32_t x = unit(a);
            for (uint32_t d = 0; d < n_out; d++)
                out.push_back(c.pbs(x, c.lut_fn([=](uint64_t v) { return part(eval(how, std::min<uint64_t>(v, a_max), scalar), d); })));
            return out;
        }
        if (b && a.size() == 1 && b->size() == 1 && pack()) {
            const uint32_t x = c.lin({{a[0], 1}, {(*b)[0], (int32_t)s.M}});
            if (c.node(x).noise <= s.budget()) {
                for (uint32_t d = 0; d < n_out; d++)
                    out.push_back(c.pbs(x, c.lut_fn([=](uint64_t v) {
                        return part(eval(how, std::min<uint64_t>(v % mm, a_max), std::min<uint64_t>(v / mm, b_max)), d);
                    })));
                return out;
            }
        }
        if (b && one_unit(a) && one_unit(*b) && (uint64_t)a_max + b_max < s.T) {
            const uint32_t wa = whole(a, a_max), wb = whole(*b, b_max);
            const bool sum = how == opname::C_ADD;
            const uint32_t x = sum ? c.lin({{wa, 1}, {wb, 1}}) : c.lin({{wa, 1}, {wb, -1}}, (int64_t)b_max);
            for (uint32_t d = 0; d < n_out; d++)
                out.push_back(c.pbs(x, c.lut_fn([=](uint64_t v) {
                    if (sum) return part(v, d);
                    return part(v >= b_max ? eval(how, v - b_max, 0) : eval(how, 0, b_max - v), d);
                })));
            return out;
        }
        if (!b) return build_clear(how, a, a_max, scalar, n_out);
        if (how == opname::C_ADD && sum_fits_low_zero(a, a_max, *b, b_max)) return sum_low_zero(a, a_max, *b, b_max, n_out);
        // the radix code on clamped digits; a sum that needs a digit more than its operands takes it from the last carry
        const std::vector<uint32_t> ca = clamped(a, a_max), cb = clamped(*b, b_max);
        const size_t n = std::max(ca.size(), cb.size());
        const std::vector<uint32_t> A = padded(ca, n), B = padded(cb, n);
        if (how == opname::C_ADD) return padded(r.add(A, B, n_out > n), n_out);
        if (how == opname::C_SUB) {
            const std::vector<uint32_t> diff = r.sub(A, B);
            const uint32_t below = c.pbs(r.sign(A, &B, 0), s.lut_equals(0));
            for (uint32_t d = 0; d < n_out; d++) out.push_back(s.gate_block(diff[d], below, false));
            return out;
        }
        if (how == opname::C_EQ || how == opname::C_NE) return {r.eq(A, &B, 0, how == opname::C_EQ)};
        return {ordered(how, r.sign(A, &B, 0))};
    }
    // A sum of two counts, the longer of three digits, whose clamps run beside the carry chain instead of before it.  The
    // three-digit operands either fill their digits or have a bound that is a multiple of M^2 (16, 32, 48 on 2-bit blocks:
    // the capacities strings usually have): then [a >= a_max] is one lookup on the third digit, the clamped operand is
    // (min(a_2, a_max / M^2), 0, 0), and it adds nothing to the low unit (two digits).  The other operand may instead be one
    // unit (one or two digits) with any bound B: its flag and its clamped digits are lookups on the unit, and where it is
    // clamped the carries of the low unit are those of (the three-digit operand) + B, which are lookups on that operand alone.
    //   level 1: the flags, min(a_2, .), a unit operand's clamped digits; [a_0 + b_0 >= M]; the state of a_1 + b_1 in
    //            {0, propagate 1, generate 2}; beside a unit operand [a_0 + B_0 >= M] and [a_lo + B >= M^2]
    //   level 2: the low digits of a three-digit operand gated by its flag; the carries out of digit 0 and of the low unit, each
    //            ANDed with the flags it holds under: one lookup on (state + [a_0 + b_0 >= M]) + 4 (flag_a + flag_b), ...
    //   level 3: message_extract of the sums with their carries, carry_extract for a fourth digit
    // -- the levels of the integer layer's add on three blocks.
    bool beside_operand(const std::vector<uint32_t>& digits, uint32_t bound) const {
        if (digits.size() > 3 || holds(digits) <= bound) return digits.size() <= 3;
        return digits.size() == 3 ? bound % (s.M * s.M) == 0 : pack();
    }
    bool sum_fits_low_zero(const std::vector<uint32_t>& a, uint32_t a_max, const std::vector<uint32_t>& b, uint32_t b_max) const {
        return std::max(a.size(), b.size()) == 3 && beside_operand(a, a_max) && beside_operand(b, b_max) &&
               (holds(a) > a_max || holds(b) > b_max) && s.T >= 16 && 2 * s.M <= s.T;
    }
    std::vector<uint32_t> sum_low_zero(const std::vector<uint32_t>& a, uint32_t a_max, const std::vector<uint32_t>& b, uint32_t b_max, uint32_t n_out) {
        const uint32_t mm = s.M, bits = s.bits_per_block, zero = c.trivial(0);
        const uint64_t unit_mod = (uint64_t)mm * mm;
        struct Side {
            std::vector<uint32_t> raw;        // three digits, as they came
            uint32_t flag, high, bound;       // [n >= bound]; the third digit as it enters the sum
            bool unit;                        // one unit with a clamp: `low` holds its clamped digits
            uint32_t low[2];
        };
        auto side = [&](const std::vector<uint32_t>& digits, uint32_t bound) {
            Side x{padded(digits, 3), zero, digits.size() == 3 ? digits[2] : zero, bound, false, {zero, zero}};
            if (holds(digits) <= bound) return x;
            if (digits.size() == 3) {
                const uint64_t top = bound / unit_mod;
                x.flag = c.pbs(digits[2], c.lut_fn([top](uint64_t v) { return (uint64_t)(v >= top); }));
                x.high = c.pbs(digits[2], c.lut_fn([top](uint64_t v) { return std::min<uint64_t>(v, top); }));
                return x;
            }
            const uint32_t u = unit(digits);
            x.unit = true;
            x.flag = c.pbs(u, c.lut_fn([bound](uint64_t v) { return (uint64_t)(v >= bound); }));
            for (uint32_t d = 0; d < digits.size(); d++)
                x.low[d] = c.pbs(u, c.lut_fn([=](uint64_t v) { return (std::min<uint64_t>(v, bound) >> (d * bits)) & (mm - 1); }));
            return x;
        };
        const Side x = side(a, a_max), y = side(b, b_max);
        const uint32_t over = c.pbs(c.lin({{x.raw[0], 1}, {y.raw[0], 1}}), c.lut_fn([mm](uint64_t v) { return (uint64_t)(v >= mm); }));
        const uint32_t state = c.pbs(c.lin({{x.raw[1], 1}, {y.raw[1], 1}}),
                                     c.lut_fn([mm](uint64_t v) { return (uint64_t)(v >= mm ? 2 : v == mm - 1 ? 1 : 0); }));
        const uint32_t flags = c.lin({{x.flag, 1}, {y.flag, 1}}, 0, 2);
        // the carries where neither operand is clamped
        std::vector<Term> into1{{c.pbs(c.lin({{over, 1}, {flags, 2}}), s.lut_equals(1)), 1}};
        std::vector<Term> into2{{c.pbs(c.lin({{state, 1}, {over, 1}, {flags, 4}}), c.lut_fn([](uint64_t v) { return (uint64_t)(v == 2 || v == 3); })), 1}};
        // ... and where the unit operand is clamped and the other one is not: the carries of (the other one) + B
        const Side* u = x.unit ? &x : y.unit ? &y : nullptr;
        if (u) {
            const Side& v = x.unit ? y : x;
            const uint64_t B = u->bound, B0 = B & (mm - 1);
            const uint32_t over_b = c.pbs(v.raw[0], c.lut_fn([=](uint64_t d) { return (uint64_t)(d + B0 >= mm); }));
            const uint32_t carry_b = c.pbs(unit({v.raw[0], v.raw[1]}), c.lut_fn([=](uint64_t d) { return (uint64_t)(d + B >= unit_mod); }));
            for (auto both : {std::make_pair(over_b, &into1), std::make_pair(carry_b, &into2)})
                both.second->push_back({c.pbs(c.lin({{both.first, 1}, {u->flag, 2}, {v.flag, 4}}), s.lut_equals(3)), 1});
        }
        std::vector<Term> sum[3];
        for (const Side* z : {&x, &y}) {
            for (int d = 0; d < 2; d++) sum[d].push_back({z->unit ? z->low[d] : s.gate_block(z->raw[d], z->flag, false), 1});
            sum[2].push_back({z->high, 1});
        }
        sum[1].insert(sum[1].end(), into1.begin(), into1.end());
        sum[2].insert(sum[2].end(), into2.begin(), into2.end());
        const uint32_t top = c.lin(sum[2]);
        std::vector<uint32_t> out{r.message_extract(c.lin(sum[0])), r.message_extract(c.lin(sum[1])), r.message_extract(top)};
        if (n_out > 3) out.push_back(r.carry_extract(top));
        return out;
    }
    uint32_t ordered(How how, uint32_t sign) {                                        // 0: below, 1: equal, 2: above
        return c.pbs(sign, c.lut_fn([how](uint64_t x) { return eval(how, x, 1); }));
    }
    // The radix code with a clear second operand k.  No clamp comes first: the digits go into the integer layer's scalar
    // forms as they are, in parallel with [a >= a_max], and where that is set the last lookup answers what a_max gives.
    //   comparisons: below its bound a' compares as a does, and from it on as a_max >= k does -- a' = a_max exactly where
    //     a >= a_max --, so only k = a_max is rewritten (eq -> ge, ne -> lt, le -> 1, gt -> 0); nothing is clamped;
    //   add: every digit of a + k is read next to [a >= a_max]; sub: next to [a < k] + 2 [a >= a_max], which also zeroes
    //     the difference below k.
    std::vector<uint32_t> build_clear(How how, const std::vector<uint32_t>& a, uint32_t a_max, uint64_t k, uint32_t n_out) {
        const bool bit = is_bit(how);
        if (how != opname::C_ADD && k > a_max) return known(eval(how, 0, 1), n_out, bit);        // a' <= a_max < k
        const uint32_t mm = s.M, bits = s.bits_per_block;
        if (bit) {
            if (k == a_max) {
                if (how == opname::C_LE || how == opname::C_GT) return known(how == opname::C_LE, 1, true);
                how = how == opname::C_EQ ? opname::C_GE : how == opname::C_NE ? opname::C_LT : how;
            }
            if (how == opname::C_EQ || how == opname::C_NE) return {r.eq(a, nullptr, k, how == opname::C_EQ)};
            return {ordered(how, r.sign(a, nullptr, k))};
        }
        const bool room = holds(a) > a_max;
        const uint32_t at_bound = room ? s.count_thermometer(a, a_max, a_max)[0] : 0;
        const uint64_t there = eval(how, a_max, k);                                   // the result from the bound on
        std::vector<uint32_t> raw, out;
        uint32_t flag = at_bound;                                                     // 1: the bound's result, 2 (sub): zero
        if (how == opname::C_ADD) {
            const size_t n = std::max<size_t>(a.size(), opname::count_digits(s.M, k));
            if (room && r.late_fits(at_bound, s.budget())) {          // the bound's sum rides on the last lookups: no level more
                RadixOps::Late late{at_bound, {}};
                for (uint32_t d = 0; d < n_out; d++) late.digits.push_back((there >> (d * bits)) & (mm - 1));
                return r.scalar_add(padded(a, n), k, n_out > n, &late);
            }
            raw = padded(r.scalar_add(padded(a, n), k, n_out > n), n_out);
        } else if (k == 0) {
            raw = a;
        } else {
            raw = r.scalar_sub(a, k);
            const uint32_t below = c.pbs(r.sign(a, nullptr, k), s.lut_equals(0));
            if (!room) {
                for (uint32_t d = 0; d < n_out; d++) out.push_back(s.gate_block(raw[d], below, false));
                return out;
            }
            if (1.0 + 5.0 * s.M * s.M <= s.budget()) flag = c.lin({{at_bound, 1}, {below, 2}}, 0, 2);    // (never both)
            else for (uint32_t& digit : raw) digit = s.gate_block(digit, below, false);                // 4-bit blocks: a lookup each
        }
        if (!room) return raw;
        for (uint32_t d = 0; d < n_out; d++) {
            const uint64_t digit = (there >> (d * bits)) & (mm - 1);
            out.push_back(c.pbs(c.lin({{raw[d], 1}, {flag, (int32_t)s.M}}),
                                c.lut_fn([=](uint64_t v) { return v / mm == 0 ? v % mm : v / mm == 1 ? digit : 0; })));
        }
        return out;
    }
};

}  // namespace fhe
