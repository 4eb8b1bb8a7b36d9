// str_regex_match.cpp -- StrOps::matches: a clear regular expression run over an encrypted string (str_ops.h, regex.h).
#include <algorithm>
#include <map>
#include <string>

#include "str_ops.h"

namespace fhe {

// ---- matches: a clear regular expression, compiled to its position automaton (regex.h), run over the characters ----
// gate AND (OR of bits) in one lookup where the sum and the gate fit the box and the noise budget side by side:
//   sum + f * gate > f       (f = number of bits; f + f^2 noise(gate))     or
//   2 * sum + gate odd, >= 3 (4 f + noise(gate)),
// whichever carries less noise; otherwise the bits are OR-ed first (grouped, any_true) and the gate joins one bit.
uint32_t StrOps::gated_or(std::vector<uint32_t> bits, uint32_t gate) {
    for (int attempt = 0; attempt < 3; attempt++) {
        const int64_t f = (int64_t)bits.size();
        double s = 0;
        for (uint32_t b : bits) s += c.node(b).noise;
        const double ng = c.node(gate).noise;
        const double noise_a = s + (double)(f * f) * ng, noise_b = 4 * s + ng;
        const bool fits_a = 2 * f < (int64_t)T && noise_a <= budget(), fits_b = 2 * f + 1 < (int64_t)T && noise_b <= budget();
        std::vector<Term> terms;
        if (fits_a && (!fits_b || noise_a <= noise_b)) {
            for (uint32_t b : bits) terms.push_back({b, 1});
            terms.push_back({gate, (int32_t)f});
            return c.pbs(c.lin(terms), c.lut_fn([f](uint64_t x) { return (uint64_t)((int64_t)x > f); }));
        }
        if (fits_b) {
            for (uint32_t b : bits) terms.push_back({b, 2});
            terms.push_back({gate, 1});
            return c.pbs(c.lin(terms), c.lut_fn([](uint64_t x) { return (uint64_t)((x & 1) && x >= 3); }));
        }
        if (bits.size() > 1) bits.assign(1, any_true(bits));    // the two-step form
        else if (c.node(bits[0]).noise > 1.0) bits[0] = fresh(bits[0]);
        else gate = fresh(gate);
    }
    return and_bits(fresh(bits[0]), fresh(gate));
}
bool StrOps::matches_fits() const {
    if (bpc % 2 || T < 16) return false;
    double nu = 0;
    for (uint32_t k = 0; k < bpc / 2; k++) nu += (double)(1u << (2 * k * bits_per_block));
    return nu <= budget();
}
uint32_t StrOps::matches(const Str& a, const regex::Automaton& g) {
    const uint32_t NONE = UINT32_MAX;               // a bit known to be 0
    const uint32_t m = g.positions(), cap = a.cap;
    // plain literals are the existing plans
    const std::string lit = g.literal();
    if (!lit.empty()) {
        const Operand text(reinterpret_cast<const uint8_t*>(lit.data()), (uint32_t)lit.size());
        if (g.sof && g.eof) return eq(a, text, true);
        if (g.sof) return starts_with(a, text);
        if (g.eof) return ends_with(a, text);
        return contains(a, text);
    }
    // the empty match: anywhere without anchors, at 0 under '^', at the hidden end under '$'
    if (g.nullable && !(g.sof && g.eof)) return c.trivial(1);

    // class bits, once per distinct class and character
    std::vector<uint32_t> class_of(m);
    std::vector<regex::ByteSet> classes;
    for (uint32_t p = 0; p < m; p++) {
        size_t k = 0;
        while (k < classes.size() && classes[k] != g.cls[p]) k++;
        if (k == classes.size()) classes.push_back(g.cls[p]);
        class_of[p] = (uint32_t)k;
    }
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> pbs_memo, cls_memo;     // (source node, table) / (class, character)
    auto lookup = [&](uint32_t node, uint32_t lut) {
        auto key = std::make_pair(node, lut);
        auto it = pbs_memo.find(key);
        return it != pbs_memo.end() ? it->second : pbs_memo[key] = c.pbs(node, lut);
    };
    std::vector<uint32_t> whole(cap, NONE), lo_nib(cap, NONE), hi_nib(cap, NONE);
    auto cls_bit = [&](uint32_t k, uint32_t i) {
        auto key = std::make_pair(k, i);
        auto it = cls_memo.find(key);
        if (it != cls_memo.end()) return it->second;
        const regex::ByteSet& S = classes[k];
        const auto& b = a.ch[i];
        uint32_t bit;
        if (whole_char_fits(b)) {
            // a whole character is one lookup input (4-bit blocks)
            if (whole[i] == NONE) whole[i] = whole_char(b);
            bit = lookup(whole[i], c.lut_fn([&S](uint64_t x) { return (uint64_t)(x < 256 && S[x]); }));
        } else {
            // nibble tables, as change_case: the high nibble names the row of the 16 x 16 membership table, the low
            // nibble answers for every row of a group at once, a third lookup joins the two.  Rows of one class are
            // told apart by the high nibble, so the bits of several groups add up to the class bit.
            if (lo_nib[i] == NONE) {
                lo_nib[i] = c.lin(nibble_terms(b, false));
                hi_nib[i] = c.lin(nibble_terms(b, true));
            }
            std::vector<uint32_t> rows;                 // distinct non-empty rows (16-bit masks over the low nibble)
            uint32_t row_of[16];
            for (uint32_t h = 0; h < 16; h++) {
                uint32_t mask = 0;
                for (uint32_t l = 0; l < 16; l++) mask |= (uint32_t)S[h * 16 + l] << l;
                size_t r = 0;
                while (r < rows.size() && rows[r] != mask) r++;
                if (mask && r == rows.size()) rows.push_back(mask);
                row_of[h] = mask ? (uint32_t)r : NONE;
            }
            uint32_t per = 1;                           // rows per group: (per + 1) 2^per values, 4^per + 1 variances
            while ((uint64_t)(per + 2) << (per + 1) <= T && 1.0 + (double)(1ull << (2 * (per + 1))) <= budget()) per++;
            std::vector<Term> parts;
            for (size_t r0 = 0; r0 < rows.size(); r0 += per) {
                const uint32_t cnt = (uint32_t)std::min<size_t>(per, rows.size() - r0);
                const uint32_t hc = lookup(hi_nib[i], c.lut_fn([&](uint64_t x) {
                    return (uint64_t)(x < 16 && row_of[x] != NONE && row_of[x] >= r0 && row_of[x] < r0 + cnt ? row_of[x] - r0 + 1 : 0); }));
                const uint32_t lc = lookup(lo_nib[i], c.lut_fn([&](uint64_t x) {
                    uint64_t v = 0;
                    for (uint32_t r = 0; r < cnt && x < 16; r++) v |= (uint64_t)((rows[r0 + r] >> x) & 1) << r;
                    return v; }));
                const uint32_t join = c.lut_fn([cnt](uint64_t x) {
                    const uint64_t row = x >> cnt, mask = x & ((1ull << cnt) - 1);
                    return (uint64_t)(row >= 1 && row <= cnt && ((mask >> (row - 1)) & 1)); });
                parts.push_back({lookup(c.lin({{hc, (int32_t)(1u << cnt)}, {lc, 1}}), join), 1});
            }
            bit = parts.empty() ? NONE : parts.size() == 1 ? parts[0].node : c.lin(parts, 0, 1);
        }
        return cls_memo[key] = bit;
    };
    // predecessors of every position
    std::vector<std::vector<uint32_t>> pred(m);
    for (uint32_t q = 0; q < m; q++)
        for (uint32_t p = 0; p < m; p++)
            if (g.follow[q][p]) pred[p].push_back(q);
    // A[p][i]: a match of the regex's prefix up to position p ends with character i
    std::vector<uint32_t> prev(m, NONE), cur(m, NONE), bits;
    std::map<uint32_t, uint32_t> end_memo;
    auto end_bit = [&](uint32_t j) {
        auto it = end_memo.find(j);
        return it != end_memo.end() ? it->second : end_memo[j] = char_is_zero(a.ch[j]);
    };
    for (uint32_t i = 0; i < cap; i++) {
        {
            Scope sc(c, owner_for(i, cap));             // a contiguous slice of the characters per rank
            for (uint32_t p = 0; p < m; p++) {
                cur[p] = NONE;
                const bool starts = g.first[p] && (i == 0 || !g.sof);
                std::vector<uint32_t> from;
                if (!starts && i > 0)
                    for (uint32_t q : pred[p])
                        if (prev[q] != NONE && std::find(from.begin(), from.end(), prev[q]) == from.end()) from.push_back(prev[q]);
                if (!starts && from.empty()) continue;
                const uint32_t cls = cls_bit(class_of[p], i);
                if (cls == NONE) continue;
                cur[p] = starts ? cls : gated_or(from, cls);
            }
        }
        std::vector<uint32_t> ends;
        for (uint32_t p = 0; p < m; p++)
            if (g.last[p] && cur[p] != NONE && std::find(ends.begin(), ends.end(), cur[p]) == ends.end()) ends.push_back(cur[p]);
        if (!ends.empty()) {
            if (g.eof && i + 1 < cap) {
                Scope sc(c, owner_for(i + 1, cap));
                bits.push_back(gated_or(ends, end_bit(i + 1)));
            } else {
                bits.insert(bits.end(), ends.begin(), ends.end());
            }
        }
        prev.swap(cur);
    }
    if (g.nullable) bits.push_back(end_bit(0));         // '^' and '$' around a nullable body: the empty string
    return fresh(any_true(bits));                       // a lone accepting bit may be a sum of class-group bits: one lookup, like every 0/1 result
}

}  // namespace fhe
