// str_split.cpp -- StrOps: counting marks, encrypted counts, the split family (str_ops.h).
#include <algorithm>

#include "str_ops.h"

namespace fhe {

// Counting marks without an integer wider than a bit: ge[q - 1][i] = [at least q of marks[0..i] are set], q = 1..Q.
// ge_1 = prefix_or(marks), ge_{q+1} = prefix_or(marks[i] AND ge_q[i - 1]); "exactly q" is the linear difference
// ge_q - ge_{q+1}.
std::vector<std::vector<uint32_t>> StrOps::count_ge(const std::vector<uint32_t>& marks, uint32_t Q) {
    std::vector<std::vector<uint32_t>> ge;
    if (Q == 0) return ge;
    const uint32_t n = (uint32_t)marks.size();
    std::vector<uint32_t> cur = prefix_or_known(marks);
    for (uint32_t q = 1;; q++) {
        ge.push_back(cur);
        if (q == Q) break;
        std::vector<uint32_t> nxt(n, c.trivial(0));
        for (uint32_t i = 1; i < n; i++) {
            Scope sc(c, owner_for(i, n));
            nxt[i] = and_bits(marks[i], cur[i - 1]);
        }
        cur = prefix_or_known(nxt);
    }
    return ge;
}
// "mask, then left-justify": the characters of s where in[i] is set (contiguous or absent), moved to the front.  The
// lead indicator NOT prefix_or(in) is monotone by construction; an empty part shifts zeros.
Str StrOps::extract_part(const Str& s, const std::vector<uint32_t>& in, uint32_t part_cap) {
    const Str g = build_str(s.cap, [&](uint32_t i, uint32_t k) { return gate_block(s.ch[i][k], in[i], true); });
    return fit(shift_left_by_leading(g, not_bits(prefix_or_known(in))), part_cap);
}
// The count of parts as little-endian base-M digits, from its unary code g_1 >= g_2 >= ... (count = sum g_v):
// digit d = sum_v g_v (digit_d(v) - digit_d(v - 1)), a value in [0, M) by construction; as many digits as max_value needs.
void StrOps::emit_count(const std::vector<uint32_t>& unary, uint32_t max_value) {
    const uint32_t n_digits = opname::count_digits(M, max_value);
    const uint32_t idm = lut_message();
    for (uint32_t d = 0; d < n_digits; d++) {
        auto dig = [&](uint32_t v) { return (int32_t)((v >> (d * bits_per_block)) & (M - 1)); };
        std::vector<Term> terms;
        for (uint32_t v = 1; v <= unary.size(); v++)
            if (dig(v) != dig(v - 1)) terms.push_back({unary[v - 1], dig(v) - dig(v - 1)});
        uint32_t digit = c.lin(terms, 0, (int64_t)M - 1);
        if (c.node(digit).noise > budget()) {
            // the differences cost their squares in noise: take the one-hot form instead, sum_v digit_d(v) [count == v],
            // every product by its own lookup (a max_parts whose sum still does not fit fails below, with the budget's message)
            terms.clear();
            for (uint32_t v = 1; v <= unary.size(); v++) {
                if (dig(v) == 0) continue;
                const uint32_t is_v = v < unary.size() ? c.lin({{unary[v - 1], 1}, {unary[v], -1}}, 0, 1) : unary[v - 1];
                terms.push_back({scale_bit(is_v, (uint32_t)dig(v)), 1});
            }
            digit = c.lin(terms, 0, (int64_t)M - 1);
        }
        if (c.node(digit).noise > 2.0) digit = c.pbs(digit, idm);
        c.output(digit);
    }
}
// ---- encrypted counts ("Encrypted counts") ----
// n arrives as D little-endian base-M digits, D the smallest with M^D > n_max (the public bound); every consumer
// works from the thermometer g[q - 1] = [n >= q], q = 1 .. n_max, so a value above the bound acts as the bound (from > 1:
// only the entries q = from .. n_max).
std::vector<uint32_t> StrOps::count_inputs(uint32_t n_max) {
    std::vector<uint32_t> digits;
    for (uint32_t d = 0; d < opname::count_digits(M, n_max); d++) digits.push_back(c.input(M - 1));
    return digits;
}
// The integer layer's scalar comparison (fhe_integer.cpp, scalar_comparison.rs:104-138 / comparator.rs:240-268) for
// every q at once: the digits are packed in pairs hi * M + lo where that fits the box and the budget.  One packed
// unit (D <= 2): [unit >= q] is one lookup per q.  More: the sign of (unit - q's unit) per unit, the most
// significant non-equal one wins, and the last pick answers [sign != less] directly.
std::vector<uint32_t> StrOps::count_thermometer(const std::vector<uint32_t>& digits, uint32_t n_max, uint32_t from) {
    const bool pack = (uint64_t)M * M <= (uint64_t)T && 1.0 + (double)M * M <= budget();
    const uint32_t per = pack ? 2 : 1;
    std::vector<uint32_t> units;
    for (size_t i = 0; i < digits.size(); i += per)
        units.push_back(pack && i + 1 < digits.size() ? c.lin({{digits[i], 1}, {digits[i + 1], (int32_t)M}}) : digits[i]);
    const uint64_t unit_mod = pack ? (uint64_t)M * M : M;
    const uint32_t sgn = lut_nonzero();                                                // odd: -1 below zero for free
    const uint32_t pick = c.lut_fn([](uint64_t x) { const uint64_t msb = (x / 4) & 3, lsb = x & 3; return msb == 1 ? lsb : msb; });
    const uint32_t pick_ge = c.lut_fn([](uint64_t x) { const uint64_t msb = (x / 4) & 3, lsb = x & 3; return (uint64_t)((msb == 1 ? lsb : msb) != 0); });
    std::vector<uint32_t> g;
    for (uint32_t q = from; q <= n_max; q++) {
        if (units.size() == 1) {
            g.push_back(c.pbs(units[0], c.lut_fn([q](uint64_t x) { return (uint64_t)(x >= q); })));
            continue;
        }
        std::vector<uint32_t> signs;       // least significant first, {0: <, 1: ==, 2: >}
        uint64_t rest = q;
        for (size_t u = 0; u < units.size(); u++, rest /= unit_mod)
            signs.push_back(c.lin({{c.pbs(c.lin({{units[u], 1}}, -(int64_t)(rest % unit_mod)), sgn, /*signed_input=*/true), 1}}, 1, 2));
        signs = tree_reduce(signs, [&](uint32_t lsb, uint32_t msb) { return c.pbs(c.lin({{msb, 4}, {lsb, 1}}), pick); }, 2);
        g.push_back(c.pbs(c.lin({{signs[1], 4}, {signs[0], 1}}), pick_ge));
    }
    return g;
}
// Selected occurrences of the pattern in s and the characters they cover: leftmost first (as replace), or rightmost
// first -- two occurrences of one length L do not overlap iff their offsets differ by at least L, so that is the same
// recurrence over the reversed match vector, hidden lengths included; cover is then rebuilt forward from sel.
// sel has s.cap entries (offsets the pattern cannot start at: known zeros).
Occurrences StrOps::select_occurrences(const Str& s, const Operand& pat, bool from_right) {
    const uint32_t n = s.cap, zero = c.trivial(0);
    std::vector<uint32_t> match, nzf;
    uint32_t m;
    bool may_overlap = true;
    if (pat.enc) {
        m = pat.enc->cap;
        for (uint32_t j = 0; j < m; j++) nzf.push_back(not_bit(char_is_zero(pat.enc->ch[j])));
        match = window_matches(s, *pat.enc, n, true);
        for (uint32_t o = 0; o < n; o++) {          // a pattern that decrypts to the empty string matches nowhere
            Scope sc(c, owner_for(o, n));
            match[o] = and_bits(match[o], nzf[0]);
        }
    } else {
        m = pat.len;
        may_overlap = has_border(pat.bytes, m);
        if (m <= n) match = window_matches_clear(s, pat.bytes, m, n - m + 1);
    }
    Occurrences oc;
    if (match.empty()) {
        oc.sel.assign(n, zero);
        oc.cover.assign(n, zero);
        return oc;
    }
    if (from_right) std::reverse(match.begin(), match.end());
    oc = occurrences(match, m, n, may_overlap, pat.enc ? &nzf : nullptr);
    if (from_right) {
        std::reverse(oc.sel.begin(), oc.sel.end());
        oc.cover = cover_from_sel(oc.sel, m, n, pat.enc ? &nzf : nullptr);
    }
    oc.sel.resize(n, zero);
    return oc;
}
void StrOps::split(const Str& s, const SplitKind& kind, const Operand& pat, uint32_t P, uint32_t part_cap, const std::vector<uint32_t>* g) {
    const uint32_t n = s.cap, zero = c.trivial(0), one = c.trivial(1);
    const uint32_t l2 = lut_equals(2);                  // numbered first, whichever kind uses it
    std::vector<std::vector<uint32_t>> in(P, std::vector<uint32_t>(n, zero));    // in[p][i]: character i belongs to part p
    std::vector<uint32_t> unary;                                                 // of the count
    if (kind.whitespace) {
        // word characters w = NOT (whitespace or null); a word starts where w rises; in_p = w AND [starts so far == p + 1]
        const std::vector<uint32_t> wz = whitespace_bits(s, true);
        std::vector<uint32_t> w = not_bits(wz), start(n);
        for (uint32_t i = 0; i < n; i++) {
            Scope sc(c, owner_for(i, n));
            start[i] = i == 0 ? w[0] : c.pbs(c.lin({{w[i], 1}, {wz[i - 1], 1}}), l2);    // (not and_bits: known bits stay in)
        }
        const auto ge = count_ge(start, P + 1);
        for (uint32_t p = 0; p < P; p++)
            for (uint32_t i = 0; i < n; i++) {
                Scope sc(c, owner_for(i, n));
                in[p][i] = and_bits(w[i], c.lin({{ge[p][i], 1}, {ge[p + 1][i], -1}}, 0, 1));
            }
        for (uint32_t v = 1; v <= P + 1; v++) unary.push_back(ge[v - 1][n - 1]);
        emit_count(unary, P + 1);
    } else {
        std::vector<uint32_t> nz(n), keep(n);
        for (uint32_t i = 0; i < n; i++) {
            Scope sc(c, owner_for(i, n));
            nz[i] = not_bit(char_is_zero(s.ch[i]));
        }
        const Occurrences oc = select_occurrences(s, pat, kind.reverse);
        for (uint32_t i = 0; i < n; i++) keep[i] = c.lin({{nz[i], 1}, {oc.cover[i], -1}}, 0, 1);     // a character outside every occurrence
        // how many selected occurrences the operation has to tell apart
        const bool drops_empty_end = kind.terminator || kind.inclusive;
        uint32_t Q = kind.once ? (kind.reverse ? 1 : 2) : kind.limited ? (kind.reverse ? P - 1 : P) : drops_empty_end ? P + 1 : P;
        Q = std::min(Q, n);                                               // (more occurrences than characters cannot be)
        std::vector<uint32_t> marks(oc.sel);
        if (kind.reverse) std::reverse(marks.begin(), marks.end());
        const auto ge = count_ge(marks, Q);
        // G(q, i) = [cF[i] >= q] (occurrences selected at offsets <= i), reverse operations: [cR[i] >= q] (offsets > i)
        auto G = [&](uint32_t q, uint32_t i) {
            if (q == 0) return one;
            if (q > Q) return zero;
            if (!kind.reverse) return ge[q - 1][i];
            return i + 1 < n ? ge[q - 1][n - 2 - i] : zero;
        };
        auto total = [&](uint32_t q) { return q == 0 ? one : q > Q ? zero : ge[q - 1][n - 1]; };   // [K >= q]
        auto exactly = [&](uint32_t q, uint32_t i) { return c.lin({{G(q, i), 1}, {G(q + 1, i), -1}}, 0, 1); };
        // e = [the string is empty, or it ends inside a selected occurrence]: the operations that drop an empty last piece
        uint32_t e = zero;
        if (drops_empty_end) {
            std::vector<uint32_t> bits{not_bit(nz[0])};
            for (uint32_t i = 0; i < n; i++) {
                int64_t v = 0;
                if (is_trivial(oc.cover[i], &v) && v == 0) continue;
                Scope sc(c, owner_for(i, n));
                bits.push_back(i + 1 < n ? c.pbs(c.lin({{oc.cover[i], 1}, {nz[i + 1], -1}}, 1), l2) : oc.cover[i]);
            }
            e = any_true(bits);
        }
        // the last piece of splitn / the second of split_once: everything from the end of occurrence number `q` on,
        // nz AND (cF >= q + 1 OR (cF == q AND NOT cover)), one lookup on (keep + 2 cover) + 3 (ge_q + ge_{q+1})
        const uint32_t l_rest = c.lut_fn([](uint64_t x) { const uint64_t u = x % 3, v = x / 3; return (uint64_t)((u == 1 && v >= 1) || (u == 2 && v == 2)); });
        auto rest_after = [&](uint32_t q, uint32_t i) {
            return c.pbs(c.lin({{nz[i], 1}, {oc.cover[i], 1}, {G(q, i), 3}, {G(q + 1, i), 3}}, 0, 8), l_rest);
        };
        const uint32_t l_incl = c.lut_fn([](uint64_t x) { const uint64_t u = x % 3, v = x / 3; return (uint64_t)(u != 0 && u == v); });
        const uint32_t l_shift = c.lut_fn([](uint64_t x) { return (uint64_t)(x == 1 || x == 5); });
        for (uint32_t p = 0; p < P; p++)
            for (uint32_t i = 0; i < n; i++) {
                Scope sc(c, owner_for(i, n));
                uint32_t bit;
                if (g) {
                    // slot q = p + 1 of an encrypted n: the ordinary piece while q < n, the rest of the string when
                    // q == n, nothing beyond -- two disjoint products, the thermometer taken into the mask lookups:
                    //   forward  keep AND [cF == q - 1] AND g_q      +  nz AND [cF >= q] AND (g_q - g_{q+1})
                    //            (rest_after(q - 1) = the ordinary piece OR everything behind occurrence q)
                    //   reverse  keep AND [cR == q - 1] AND g_{q+1}  +  nz AND [cR >= q - 1] AND (g_q - g_{q+1})
                    const uint32_t q = p + 1, g_q = (*g)[p], g_next = q < P ? (*g)[q] : zero;
                    const uint32_t is_last = c.lin({{g_q, 1}, {g_next, -1}}, 0, 1);
                    const uint32_t ordinary = and_all({keep[i], exactly(q - 1, i), kind.reverse ? g_next : g_q});
                    const uint32_t rest = and_all({nz[i], G(kind.reverse ? q - 1 : q, i), is_last});
                    bit = c.lin({{ordinary, 1}, {rest, 1}}, 0, 1);
                }
                else if (kind.once && kind.reverse) bit = p == 0 ? and_bits(nz[i], G(1, i)) : and_bits(keep[i], exactly(0, i));
                else if (kind.once) bit = p == 0 ? and_bits(keep[i], exactly(0, i)) : rest_after(1, i);
                else if (kind.limited && p == P - 1) bit = kind.reverse ? and_bits(nz[i], G(P - 1, i)) : rest_after(P - 1, i);
                else if (kind.inclusive) {    // (NOT cover AND cF == p) OR (cover AND cF == p + 1), on (keep + 2 cover) + 3 (eq_p + 2 eq_{p+1})
                    const uint32_t x = c.lin({{nz[i], 1}, {oc.cover[i], 1}, {G(p, i), 3}, {G(p + 1, i), 3}, {G(p + 2, i), -6}}, 0, 8);
                    bit = c.node(x).noise <= budget() ? c.pbs(x, l_incl)      // (54 nominal variances and more; else the two terms apart)
                                                      : c.lin({{and_bits(keep[i], exactly(p, i)), 1}, {and_bits(oc.cover[i], exactly(p + 1, i)), 1}}, 0, 1);
                }
                else if (kind.terminator && kind.reverse)      // cR == p + e: e picks between "exactly p" and "exactly p + 1"
                    bit = and_bits(keep[i], c.pbs(c.lin({{G(p, i), 1}, {G(p + 1, i), 1}, {G(p + 2, i), -2}, {e, 3}}, 0, 5), l_shift));
                else bit = and_bits(keep[i], exactly(p, i));
                in[p][i] = bit;
            }
        if (kind.once) {
            c.output(total(1));                                           // found
        } else {
            if (drops_empty_end) {
                // piece p exists iff K >= p + 1, or K == p and the last piece is not empty: on (ge_p + ge_{p+1}) + 3 e
                const uint32_t l_ex = c.lut_fn([](uint64_t x) { return (uint64_t)(x == 1 || x == 2 || x == 5); });
                for (uint32_t p = 0; p <= P; p++)
                    unary.push_back(c.pbs(c.lin({{total(p), 1}, {total(p + 1), 1}, {e, 3}}, 0, 5), l_ex));
            } else if (g) {
                for (uint32_t v = 1; v <= P; v++) unary.push_back(and_bits((*g)[v - 1], total(v - 1)));    // min(1 + K, n)
            } else {
                for (uint32_t v = 1; v <= (kind.limited ? P : P + 1); v++) unary.push_back(total(v - 1));   // 1 + K, capped
            }
            emit_count(unary, P + 1);
        }
    }
    for (uint32_t p = 0; p < P; p++) {
        Scope sc(c, owner_for(p, P));                                     // one rank per part
        emit(extract_part(s, in[p], part_cap));
    }
}

}  // namespace fhe
