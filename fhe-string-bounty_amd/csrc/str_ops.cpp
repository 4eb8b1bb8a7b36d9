// str_ops.cpp -- StrOps: noise grouping, reductions, block and character comparisons, gates and selects, the barrel
// shifter, concatenation, case, whitespace and trims, len (str_ops.h).
#include <algorithm>
#include <map>

#include "str_ops.h"

namespace fhe {

// The noise of sum_t coeff_t * node_t as Circuit::lin will build it: sources that several terms share add up by
// coefficient before they are squared (a LIN node is flattened onto inputs and lookup outputs).  It passes the terms'
// own noise added up where the terms are sums over the same lookup outputs: the bits `nz - cover` of a selection taken
// from the right with a clear pattern of 6 characters and more share up to 8 of them.
double StrOps::sum_noise(const std::vector<Term>& terms) const {
    std::map<uint32_t, int64_t> by_source;
    for (const Term& t : terms) {
        const Node& n = c.node(t.node);
        if (n.kind == Node::LIN) for (const Term& u : n.terms) by_source[u.node] += (int64_t)t.coeff * u.coeff;
        else by_source[t.node] += t.coeff;
    }
    double nu = 0;
    for (const auto& kv : by_source) nu += (double)kv.second * kv.second * c.node(kv.first).noise;
    return nu;
}
std::vector<std::vector<Term>> StrOps::term_groups(const std::vector<Term>& terms, size_t max_terms) const {
    std::vector<std::vector<Term>> out;
    double nu = 0;
    for (const Term& t : terms) {
        const double add = (double)t.coeff * t.coeff * c.node(t.node).noise;
        if (out.empty() || out.back().size() >= max_terms || (nu + add > budget() && !out.back().empty())) {
            out.emplace_back();
            nu = 0;
        }
        out.back().push_back(t);
        nu += add;
    }
    return out;
}
// ---- reductions of 0/1 blocks ----
// are_all_comparisons_block_true (scalar_comparison.rs:147-191) / is_at_least_one_comparisons_block_true
// (scalar_comparison.rs:200-233) on one rank: chunks of up to msg*carry - 1 bits (fewer if the
// noise budget says so) are summed and sent through `x == chunk_len` / `x != 0`, repeated to one bit
// Default (not the reference-shaped plans): chunks of T bits where that saves a lookup level -- the sum T is the
// padding bit, answered consistently by a table of -/+ delta/2 (Circuit::pbs_full_box).  AND over a 16-char pattern
// and OR over up to 256 offsets then take one level less each (PARAM_MESSAGE_2_CARRY_2: contains 16-in-256 7 -> 5 levels).
uint32_t StrOps::reduce_local(std::vector<uint32_t> bits, bool all) {
    const uint32_t nz = lut_nonzero();
    while (bits.size() > 1) {
        std::vector<Term> terms;
        for (uint32_t b : bits) terms.push_back({b, 1});
        std::vector<uint32_t> next;
        for (const auto& g : term_groups(terms, full_box_reduce ? T : T - 1)) {
            const size_t len = g.size();
            if (len == T) { next.push_back(c.pbs_full_box(c.lin(g), all)); continue; }
            next.push_back(c.pbs(c.lin(g), all ? lut_equals(len) : nz));
        }
        bits.swap(next);
    }
    return bits[0];
}
// The same over several ranks: every rank first reduces the bits it owns to ONE block,
// only those blocks travel (one all-gather), and the last PBS combines them.
uint32_t StrOps::reduce_bits(const std::vector<uint32_t>& bits, bool all) {
    if (bits.empty()) return c.trivial(all ? 1 : 0);
    if (world <= 1 || c.owner_hint() >= 0) return reduce_local(bits, all);
    std::map<int, std::vector<uint32_t>> by_owner;
    for (uint32_t b : bits) by_owner[c.owner_of(b)].push_back(b);
    if (by_owner.size() == 1 && by_owner.begin()->first < 0) return reduce_local(bits, all);
    std::vector<uint32_t> partial;
    for (auto& kv : by_owner) {
        if (kv.first < 0) { partial.insert(partial.end(), kv.second.begin(), kv.second.end()); continue; }
        Scope sc(c, kv.first);
        partial.push_back(reduce_local(kv.second, all));
    }
    return reduce_local(partial, all);
}
// message_extract (shortint/server_key/mod.rs: x -> x % msg_mod) of a block that carries more than
// nominal noise (a sum of ciphertexts): back to NoiseLevel::NOMINAL for one PBS
uint32_t StrOps::fresh(uint32_t block) {
    if (c.node(block).noise <= 1.0) return block;
    auto it = fresh_memo.find(block);
    if (it != fresh_memo.end()) return it->second;
    return fresh_memo[block] = c.pbs(block, lut_message());
}
// ---- block-level comparisons ----
// bivariate LUT on lhs*M + rhs (bivariate_pbs.rs:71-96,167-182)
uint32_t StrOps::block_eq(uint32_t a, uint32_t b, bool want_equal) {
    const uint32_t m = M;
    if ((double)M * M * c.node(a).noise + c.node(b).noise > budget()) a = fresh(a);     // noisy operands
    if ((double)M * M * c.node(a).noise + c.node(b).noise > budget()) b = fresh(b);
    const uint32_t l = c.lut_fn([m, want_equal](uint64_t x) {
        const uint64_t lhs = (x / m) % m, rhs = (x % m) % m;
        return (uint64_t)((lhs == rhs) == want_equal);
    });
    return c.pbs(c.lin({{a, (int32_t)M}, {b, 1}}), l);
}
// Two blocks per PBS: (lo_a + M*hi_a) - (lo_b + M*hi_b) lies in (-T, T); as a torus value it uses
// the padding bit for the sign, and a negacyclic table with f(0) = 1, f(1..T-1) = 0 returns
// -f(x - T) = 0 on the negative side as well, so one lookup answers "both blocks equal".
// (Only equality can be read this way: a table that is 1 on both signs cannot be negacyclic.)
uint32_t StrOps::packed_pair_eq(uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b) {
    return c.pbs(c.lin({{lo_a, 1}, {hi_a, (int32_t)M}, {lo_b, -1}, {hi_b, -(int32_t)M}}), lut_equals(0), /*signed_input=*/true);
}
bool StrOps::packed_pair_fits(uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b) const {
    const double m2 = (double)M * M;
    return c.node(lo_a).noise + c.node(lo_b).noise + m2 * (c.node(hi_a).noise + c.node(hi_b).noise) <= budget();
}
std::vector<uint32_t> StrOps::char_eq_bits(const std::vector<uint32_t>& x, const std::vector<uint32_t>& y) {
    // packed form only where its 2(1 + M^2) nominal variances fit the parameter set's noise budget
    // (noise_model.h); otherwise the reference's bivariate shape, M^2 + 1
    bool packed = packed_compare && bpc % 2 == 0;
    for (uint32_t k = 0; packed && k + 1 < bpc; k += 2) packed = packed_pair_fits(x[k], x[k + 1], y[k], y[k + 1]);
    std::vector<uint32_t> out;
    if (packed) {
        for (uint32_t k = 0; k + 1 < bpc; k += 2) out.push_back(packed_pair_eq(x[k], x[k + 1], y[k], y[k + 1]));
    } else {
        for (uint32_t k = 0; k < bpc; k++) out.push_back(block_eq(x[k], y[k], true));
    }
    return out;
}
// pack_block_chunk + scalar LUT (scalar_comparison.rs:104-138,312-336,431-452): two blocks of a
// char packed as hi*M + lo, compared with the clear value packed the same way.
std::vector<uint32_t> StrOps::char_scalar_bits(const std::vector<uint32_t>& blocks, uint8_t v, bool want_equal) {
    std::vector<uint32_t> out;
    for (uint32_t b = 0; b + 1 < bpc; b += 2) {
        const uint32_t clear = clear_block(v, b + 1) * M + clear_block(v, b);
        const uint32_t l = c.lut_fn([clear, want_equal](uint64_t x) { return (uint64_t)((x == clear) == want_equal); });
        out.push_back(c.pbs(c.lin({{blocks[b + 1], (int32_t)M}, {blocks[b], 1}}), l));
    }
    return out;
}
uint32_t StrOps::char_is_zero(const std::vector<uint32_t>& blocks) {
    const uint32_t per = (T - 1) / (M - 1);
    const uint32_t tt = T;
    const uint32_t z = c.lut_fn([tt](uint64_t x) { return (uint64_t)((x % tt) == 0); });
    std::vector<uint32_t> bits;
    for (size_t i = 0; i < blocks.size(); i += per) {
        std::vector<Term> terms;
        for (size_t j = i; j < std::min(blocks.size(), i + per); j++) terms.push_back({blocks[j], 1});
        bits.push_back(c.pbs(c.lin(terms), z));
    }
    return all_true(bits);
}
std::vector<Term> StrOps::nibble_terms(const std::vector<uint32_t>& b, bool high) const {
    const uint32_t half = bpc / 2;   // blocks per nibble (2 for 2-bit blocks)
    std::vector<Term> terms;
    for (uint32_t k = 0; k < half; k++) terms.push_back({b[(high ? half : 0) + k], (int32_t)(1u << (k * bits_per_block))});
    return terms;
}
uint32_t StrOps::classify_nibbles(const std::vector<uint32_t>& b, uint32_t hi_lut, uint32_t lo_lut, uint32_t comb) {
    const uint32_t hc = c.pbs(c.lin(nibble_terms(b, true)), hi_lut);
    const uint32_t lc = c.pbs(c.lin(nibble_terms(b, false)), lo_lut);
    return c.pbs(c.lin({{hc, 4}, {lc, 1}}), comb);
}
// ---- case conversion (docs/tutorials/ascii_fhe_string.md:88-131 semantics) ----
// to_lower: c in ['A','Z'] -> c + 32 ; to_upper: c in ['a','z'] -> c - 32.  32 = 2 * 16 only
// touches bit 5, i.e. block (5 / bits_per_block); letters never carry out of that block.
Str StrOps::change_case(const Str& s, bool to_lower) {
    const uint32_t lo_first = to_lower ? 'A' : 'a', lo_last = to_lower ? 'Z' : 'z';
    const uint32_t hiA = lo_first >> 4, hiB = lo_last >> 4;          // 4 / 5  or  6 / 7
    const uint32_t loA = lo_first & 15, loB = lo_last & 15;         // 1 and 10
    const uint32_t blk = 5 / bits_per_block, bit_in_blk = 5 % bits_per_block;
    const uint32_t addv = 1u << bit_in_blk;
    // level 1: classify high nibble (0 / 1 = first row / 2 = second row) and low nibble
    // (bit0 = lo >= loA, bit1 = lo <= loB); level 2: combine into addv * is_letter
    const uint32_t hi_lut = c.lut_fn([hiA, hiB](uint64_t x) { return (uint64_t)(x == hiA ? 1 : (x == hiB ? 2 : 0)); });
    const uint32_t lo_lut = c.lut_fn([loA, loB](uint64_t x) { return (uint64_t)((x >= loA ? 1 : 0) | (x <= loB ? 2 : 0)); });
    const uint32_t comb = c.lut_fn([addv](uint64_t x) {
        const uint64_t a = x / 4, b = x % 4;
        const bool is = (a == 1 && (b & 1)) || (a == 2 && (b & 2));
        return (uint64_t)(is ? addv : 0);
    });
    // whole-char form: the block that holds bit 5, already converted
    const uint32_t Mv = M, shift = blk * bits_per_block;
    const uint32_t whole_lut = c.lut_fn([=](uint64_t x) {
        const uint64_t block = (x >> shift) & (Mv - 1);
        const bool is = x >= lo_first && x <= lo_last;
        return is ? (to_lower ? block + addv : block - addv) : block;
    });
    Str out = blank(s.cap);
    for (uint32_t i = 0; i < s.cap; i++) {
        Scope sc(c, owner_for(i, s.cap));
        const auto& b = s.ch[i];
        out.ch[i] = b;
        if (whole_char_fits(b)) {
            out.ch[i][blk] = c.pbs(whole_char(b), whole_lut);
            continue;
        }
        const uint32_t delta = classify_nibbles(b, hi_lut, lo_lut, comb);
        out.ch[i][blk] = c.lin({{b[blk], 1}, {delta, to_lower ? 1 : -1}}, 0, (int64_t)M - 1);   // letters never carry
    }
    return out;
}
// ---- whitespace trimming ----
// wz[i] = [s[i] is ASCII whitespace (9..13, 32)] (+ [s[i] == 0] when null_too): 3 PBS per char
std::vector<uint32_t> StrOps::whitespace_bits(const Str& s, bool null_too) {
    const uint32_t hi_lut = c.lut_fn([](uint64_t x) { return (uint64_t)(x == 0 ? 1 : (x == 2 ? 2 : 0)); });
    const uint32_t lo_lut = c.lut_fn([null_too](uint64_t x) {
        const bool row0 = (x >= 9 && x <= 13) || (null_too && x == 0);
        return (uint64_t)((row0 ? 1 : 0) | (x == 0 ? 2 : 0));
    });
    const uint32_t comb = c.lut_fn([](uint64_t x) {
        const uint64_t a = x / 4, b = x % 4;
        return (uint64_t)(((a == 1 && (b & 1)) || (a == 2 && (b & 2))) ? 1 : 0);
    });
    const uint32_t whole_lut = c.lut_fn([null_too](uint64_t x) {
        return (uint64_t)(((x >= 9 && x <= 13) || x == 32 || (null_too && x == 0)) ? 1 : 0);
    });
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < s.cap; i++) {
        Scope sc(c, owner_for(i, s.cap));
        if (whole_char_fits(s.ch[i])) out.push_back(c.pbs(whole_char(s.ch[i]), whole_lut));
        else out.push_back(classify_nibbles(s.ch[i], hi_lut, lo_lut, comb));
    }
    return out;
}
// block * bit (bit in {0,1}) : LUT on bit + 2*block  (noise: 1 + 2*level(block))
uint32_t StrOps::gate_block(uint32_t block, uint32_t bit, bool keep_if_set) {
    int64_t v = 0;
    if (is_trivial(block, &v) && v == 0) return block;                       // 0 * anything
    if (is_trivial(bit, &v)) return ((v != 0) == keep_if_set) ? block : c.trivial(0);
    const uint32_t m2 = 2 * M;
    const uint32_t l = c.lut_fn([keep_if_set, m2](uint64_t x) {
        return (uint64_t)((x < m2 && ((x & 1) != 0) == keep_if_set) ? x >> 1 : 0);
    });
    return c.pbs(c.lin({{bit, 1}, {block, 2}}), l);
}
// sel ? b : a for two blocks in [0, M-1] in ONE lookup (default plans): a + sel * (b - a), the product read off
// (b - a) + (M-1) + (2M-1) sel in [0, 4M-3].  The result keeps a's noise plus one nominal variance (the two-gate form
// returns two fresh lookups): callers that chain it clean the blocks at the end (fresh()).  Falls back to the two
// gates where the packing does not fit the box or the budget (PARAM_MESSAGE_4_CARRY_4: (2M-1)^2 = 961 variances).
uint32_t StrOps::select_block(uint32_t a, uint32_t b, uint32_t sel, uint32_t hi) {
    int64_t v = 0;
    if (is_trivial(sel, &v)) return v ? b : a;
    const uint32_t D = 2 * hi + 1;                           // distinct values of b - a, both in [0, hi]
    const uint32_t x = full_box_reduce && 2 * D <= T ? c.lin({{b, 1}, {a, -1}, {sel, (int32_t)D}}, (int64_t)hi) : UINT32_MAX;
    if (x == UINT32_MAX || c.node(x).noise > budget())       // (noise of the combination as built: shared sources add up)
        return c.lin({{gate_block(a, sel, false), 1}, {gate_block(b, sel, true), 1}}, 0, hi);
    const uint32_t l = c.lut_fn([D, hi](uint64_t y) { return (uint64_t)(y >= 2 * D ? hi : (y / D ? y % D : hi)); });
    return c.lin({{a, 1}, {c.pbs(x, l), 1}}, -(int64_t)hi, (int64_t)hi);
}
// trim_end: zero every char from the last non-whitespace one onwards
Str StrOps::trim_end(const Str& s) {
    std::vector<uint32_t> wz = whitespace_bits(s, true), nw(s.cap);
    for (uint32_t i = 0; i < s.cap; i++) nw[s.cap - 1 - i] = not_bit(wz[i]);   // reversed, 1 = real char
    std::vector<uint32_t> keep_rev = prefix_or(nw);        // keep[i] = OR_{j >= i} nonws[j]
    return build_str(s.cap, [&](uint32_t i, uint32_t k) { return gate_block(s.ch[i][k], keep_rev[s.cap - 1 - i], true); });
}
// trim_start: shift left by the (encrypted) number of leading whitespace chars with a barrel
// shifter; stage t shifts by 2^t iff the first 2^t chars are all whitespace
Str StrOps::trim_start(const Str& s) {
    const std::vector<uint32_t> seen = prefix_or(not_bits(whitespace_bits(s, false)));   // seen[i] = some non-ws char in [0, i]
    return shift_left_by_leading(s, not_bits(seen));                                      // lead[i] = chars 0..i all whitespace
}
// Shift `s` left by the number of leading ones of the monotone indicator lead (lead[i] = 1 for
// i < z, 0 after): barrel shifter, stage t shifts by 2^t iff lead[2^t - 1] (i.e. z >= 2^t), the
// indicator shifts along with the string.  (cmux per block: integer/server_key/radix_parallel/cmux.rs)
Str StrOps::shift_left_by_leading(const Str& s, std::vector<uint32_t> lead) {
    Str cur = s;
    int top = 0;
    while ((1u << (top + 1)) <= s.cap) top++;
    for (int t = top; t >= 0; t--) {
        const uint32_t sh = 1u << t;
        if (sh > s.cap) continue;
        const uint32_t sel = lead[sh - 1];
        int64_t sv = 0;
        if (is_trivial(sel, &sv) && sv == 0) continue;       // the indicator is known to be shorter
        Str nxt = blank(s.cap);
        std::vector<uint32_t> nlead(s.cap);
        for (uint32_t i = 0; i < s.cap; i++) {
            for (size_t k = 0; k < cur.ch[i].size(); k++) {
                if (i + sh < s.cap) nxt.ch[i].push_back(select_block(cur.ch[i][k], cur.ch[i + sh][k], sel, M - 1));
                else nxt.ch[i].push_back(gate_block(cur.ch[i][k], sel, false));
            }
            // the monotone indicator shifts with the string
            // (a fresh bit every stage -- it is the next stages' selector, whose noise is weighted (2M-1)^2 above:
            //  one lookup on lead[i] + 2 lead[i + sh] + 4 sel)
            // (the noise of the combination as built: operands that share sources, e.g. lead[i] == sel, add up)
            const uint32_t packed3 = i + sh < s.cap && full_box_reduce && T >= 8
                                         ? c.lin({{lead[i], 1}, {lead[i + sh], 2}, {sel, 4}}) : UINT32_MAX;
            if (packed3 != UINT32_MAX && c.node(packed3).noise <= budget()) {
                int64_t va = 0, vb = 0;
                const bool ta = is_trivial(lead[i], &va), tb = is_trivial(lead[i + sh], &vb);
                if (ta && tb && va == vb) nlead[i] = lead[i];
                else nlead[i] = c.pbs(packed3, c.lut_fn([](uint64_t x) { return (uint64_t)((x & 4) ? (x >> 1) & 1 : x & 1); }));
            } else
            nlead[i] = i + sh < s.cap ? select_block(lead[i], lead[i + sh], sel, 1) : c.lin({{gate_block(lead[i], sel, false), 1}}, 0, 1);
        }
        cur = nxt;
        lead = nlead;
    }
    // blocks that went through select_block stages carry one nominal variance per stage: back to a fresh lookup's
    for (auto& chr : cur.ch)
        for (uint32_t& b : chr)
            if (c.node(b).noise > 2.0) b = fresh(b);
    return cur;
}
// concat: a ++ b without a's padding.  b is parked behind a's full capacity and shifted left by the
// number of null characters at the end of a (monotone indicator read from the end of a); the result
// (capacity a.cap + b.cap) is a + shifted(b): wherever b lands, a is null.
// with_occ: two left-justified strings whose per-slot occupancy bits are known (occ): the shift is by the left one's
// free slots, the occupancy travels as one more block.  No char_is_zero needed.
Str StrOps::concat(const Str& a, const Str& b, bool with_occ) {
    const uint32_t zero = c.trivial(0), nb = bpc + (with_occ ? 1 : 0);
    Str u = blank(a.cap + b.cap);
    for (uint32_t i = 0; i < a.cap; i++) u.ch[i].assign(nb, zero);
    for (uint32_t j = 0; j < b.cap; j++) {
        u.ch[a.cap + j].assign(b.ch[j].begin(), b.ch[j].begin() + bpc);
        if (with_occ) u.ch[a.cap + j].push_back(b.occ[j]);
    }
    std::vector<uint32_t> lead(u.cap, zero);             // 1 while in a's free tail / still in a's padding
    for (uint32_t t = 0; t < a.cap; t++) lead[t] = with_occ ? not_bit(a.occ[a.cap - 1 - t]) : char_is_zero(a.ch[a.cap - 1 - t]);
    const Str v = shift_left_by_leading(u, lead);
    Str out = blank(u.cap, with_occ);
    for (uint32_t i = 0; i < u.cap; i++) {
        for (uint32_t k = 0; k < bpc; k++)
            out.ch[i].push_back(i < a.cap ? c.lin({{a.ch[i][k], 1}, {v.ch[i][k], 1}}, 0, M - 1) : v.ch[i][k]);
        if (with_occ) out.occ[i] = i < a.cap ? c.lin({{a.occ[i], 1}, {v.ch[i][bpc], 1}}, 0, 1) : v.ch[i][bpc];
    }
    return out;
}
Str StrOps::fit(const Str& r, uint32_t cap) {
    Str out = blank(cap);
    const uint32_t zero = c.trivial(0);
    for (uint32_t i = 0; i < cap; i++) {
        if (i < r.cap) out.ch[i].assign(r.ch[i].begin(), r.ch[i].begin() + bpc);
        else out.ch[i].assign(bpc, zero);
    }
    return out;
}
// ---- gates on bits ----
uint32_t StrOps::and_bits(uint32_t a, uint32_t b) {
    int64_t v = 0;
    if (is_trivial(a, &v)) return v ? b : a;
    if (is_trivial(b, &v)) return v ? a : b;
    return c.pbs(c.lin({{a, 1}, {b, 1}}), lut_equals(2));
}
uint32_t StrOps::scale_bit(uint32_t bit, uint32_t v) {
    if (v == 0) return c.trivial(0);
    int64_t b = 0;
    if (is_trivial(bit, &b)) return c.trivial(b ? (int64_t)v : 0);
    return c.pbs(bit, c.lut_fn([v](uint64_t x) { return (uint64_t)(x == 1 ? v : 0); }));
}
uint32_t StrOps::and_all(const std::vector<uint32_t>& bits) {
    std::vector<Term> terms;
    for (uint32_t b : bits) {
        int64_t v = 0;
        if (!is_trivial(b, &v)) terms.push_back({b, 1});
        else if (v == 0) return c.trivial(0);
    }
    if (terms.empty()) return c.trivial(1);
    if (terms.size() == 1) return terms[0].node;
    return c.pbs(c.lin(terms), lut_equals(terms.size()));
}
// ---- combining results ----
uint32_t StrOps::combine_bits(const std::vector<uint32_t>& bits, opname::How how) {
    std::vector<uint32_t> open;
    int64_t ones = 0;
    for (uint32_t b : bits) {
        int64_t v = 0;
        if (!is_trivial(b, &v)) open.push_back(b);
        else if (how == opname::L_XOR) ones += v & 1;
        else if ((v != 0) != (how == opname::L_AND)) return c.trivial(how == opname::L_AND ? 0 : 1);    // AND with 0, OR with 1
    }
    if (how != opname::L_XOR) return open.empty() ? c.trivial(how == opname::L_AND ? 1 : 0) : reduce_bits(open, how == opname::L_AND);
    // parity: sums of up to T - 1 bits, each read by x & 1, then the parity of those
    const uint32_t odd = c.lut_fn([](uint64_t x) { return x & 1; });
    while (open.size() > 1) {
        std::vector<Term> terms;
        for (uint32_t b : open) terms.push_back({b, 1});
        auto groups = term_groups(terms, T - 1);
        if (groups.size() == open.size()) groups.assign(1, terms);      // no two fit one lookup: the build fails on the budget, with its message
        std::vector<uint32_t> next;
        for (const auto& g : groups) next.push_back(g.size() == 1 ? g[0].node : c.pbs(c.lin(g), odd));
        open.swap(next);
    }
    if (open.empty()) return c.trivial(ones & 1);
    return (ones & 1) ? not_bit(open[0]) : open[0];
}
Str StrOps::select(uint32_t sel, const Str& a, const Str& b, uint32_t cap) {
    const Str fa = fit(a, cap), fb = fit(b, cap);
    return build_str(cap, [&](uint32_t i, uint32_t k) {
        Scope sc(c, owner_for(i, cap));
        if (i >= a.cap) return gate_block(fb.ch[i][k], sel, false);
        if (i >= b.cap) return gate_block(fa.ch[i][k], sel, true);
        return select_block(fb.ch[i][k], fa.ch[i][k], sel, M - 1);
    });
}
std::vector<uint32_t> StrOps::select_digits(uint32_t sel, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
    std::vector<uint32_t> out;
    for (size_t d = 0; d < std::max(a.size(), b.size()); d++)
        out.push_back(d >= a.size() ? gate_block(b[d], sel, false) : d >= b.size() ? gate_block(a[d], sel, true) : select_block(b[d], a[d], sel, M - 1));
    return out;
}
void StrOps::settle_combined(std::vector<uint32_t>& blocks, uint32_t anchor) {
    for (uint32_t& b : blocks) {
        int64_t known = 0;
        const Node& n = c.node(b);
        bool looked_up = n.kind == Node::PBS;
        for (const Term& t : n.terms) looked_up |= n.kind == Node::LIN && c.node(t.node).kind == Node::PBS;
        if (is_trivial(b, &known)) b = c.pbs(anchor, c.lut_fn([known](uint64_t) { return (uint64_t)known; }));
        else if (!looked_up) b = c.pbs(b, lut_message());
    }
}
// len = offset of the first null char (cap when there is none): found bit is always 1
std::vector<uint32_t> StrOps::len(const Str& s, uint32_t n_digits) {
    std::vector<uint32_t> z;
    for (uint32_t i = 0; i < s.cap; i++) z.push_back(char_is_zero(s.ch[i]));
    z.push_back(c.trivial(1));
    const std::vector<uint32_t> found_and_digits = find_from_matches(z, n_digits);
    return std::vector<uint32_t>(found_and_digits.begin() + 1, found_and_digits.end());
}


}  // namespace fhe
