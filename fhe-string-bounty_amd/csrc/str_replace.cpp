// str_replace.cpp -- StrOps: occurrence selection (recurrence and blocked scan), cover, replace (str_ops.h).
#include <algorithm>
#include <cstring>
#include <map>

#include "str_ops.h"

namespace fhe {

// The leftmost non-overlapping occurrences as a BLOCKED SCAN (round 4).  The recurrence below is a chain over the offsets,
// one lookup level per two of them (n / 2 levels: 0.33 s for 256 characters on PARAM_MESSAGE_2_CARRY_2, each level a single-
// PBS latency).  Its state is small: r[o] = how many more characters the occurrence selected before o still covers, in
// [0, m).  One step is ONE lookup,   r[o+1] = (r[o] == 0) ? g[o] : r[o] - 1   on   x = r[o] + m g[o],
// with g[o] = match[o] * (L - 1) (L = the pattern's length: m, or the hidden number of non-null characters of a padded
// encrypted pattern -- then g costs one lookup per offset, off the chain).  Blocks of B offsets run their chains for every
// possible incoming state at once (m hypotheses, constants at the block's start), the true state then hops from block to
// block through the blocks' state maps (m lookups per hop: select F_b[R_b] by the encrypted R_b), and every block re-runs
// its chain from its true incoming state.  Depth 2 B + n / B instead of n / 2 -- B + n / B with two offsets per chain step
// (1024 characters, 4-character pattern: 66 levels instead of 511) --, about (m + 1) n chain lookups instead of n.  sel[o] = [r[o] == 0 and match[o]] and cover[o] = [r[o] > 0 or
// match[o]] are read off x' = r[o] + m match[o] afterwards.  Needs m^2 <= T (hidden length) or 2 m <= T; the recurrence
// stays for longer patterns, short strings and where the noise does not fit.
bool StrOps::occurrences_scan(const std::vector<uint32_t>& match, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf, Occurrences& oc) {
    const uint32_t n = (uint32_t)match.size();
    if (!blocked_scan || m < 2 || n < 48) return false;
    const bool hidden = nzf != nullptr;
    if (hidden ? (uint64_t)m * m > T : 2ull * m > T) return false;
    for (uint32_t o = 0; o < n; o++) if (is_trivial(match[o])) return false;      // (plans with clear operands: keep the recurrence)
    const uint32_t mm = m;
    std::vector<uint32_t> g(n);
    if (hidden) {
        std::vector<Term> t;
        double nu = 0;
        for (uint32_t j = 1; j < m; j++) { t.push_back({(*nzf)[j], 1}); nu += c.node((*nzf)[j]).noise; }
        const uint32_t lm1 = c.lin(t, 0, m - 1);          // L - 1 (padding sits at the end; an empty pattern matches nowhere)
        const uint32_t gl = c.lut_fn([mm](uint64_t x) { return (x & 1) ? std::min<uint64_t>(x >> 1, mm - 1) : (uint64_t)0; });
        for (uint32_t o = 0; o < n; o++) {
            if (c.node(match[o]).noise + 4 * nu > budget()) return false;
            Scope sc(c, owner_for(o, n));
            g[o] = c.pbs(c.lin({{match[o], 1}, {lm1, 2}}), gl);
        }
        if (1.0 + (double)m * m * 1.0 + (double)m > budget()) return false;    // chain input: r (up to m outputs summed) + m g
    } else {
        g = match;
        for (uint32_t o = 0; o < n; o++)
            if ((double)m + (double)m * m * c.node(match[o]).noise > budget()) return false;
    }
    const uint32_t step = hidden ? c.lut_fn([mm](uint64_t x) { return x % mm == 0 ? x / mm : x % mm - 1; })
                                 : c.lut_fn([mm](uint64_t x) { const uint64_t r = x % mm; return r == 0 ? (x / mm ? (uint64_t)mm - 1 : (uint64_t)0) : r - 1; });
    const uint32_t n_ext = std::min(n_chars, n + m - 1);      // past the last offset an occurrence may still run
    const uint32_t zero = c.trivial(0);
    auto g_at = [&](uint32_t o) { return o < n ? g[o] : zero; };
    // Two offsets per chain step where the box and the noise allow it: x = r + m g[o] + W g[o+1], W = m^2 (hidden length:
    // g in [0, m)) or 2 m (known length: g is the match bit) -- known length m = 4 fills the 16 values of PARAM_MESSAGE_2_CARRY_2
    // exactly.  The state between the two (needed for sel / cover on the true chains only) is one more lookup off the chain.
    const uint32_t W = hidden ? m * m : 2 * m;
    const bool pairs = (hidden ? (uint64_t)m * m * m : 4ull * m) <= T && (double)m + (double)m * m + (double)W * W <= budget();
    auto one = [mm, hidden](uint64_t r, uint64_t gv) -> uint64_t { return r == 0 ? (hidden ? gv : (gv ? (uint64_t)mm - 1 : (uint64_t)0)) : r - 1; };
    const uint32_t step2 = !pairs ? 0u : c.lut_fn([mm, W, one](uint64_t x) { return one(one(x % mm, (x % W) / mm), x / W); });
    // state entering lo, lo + 1, ..., hi (hi - lo + 1 values; only the last one unless `all`) from the state `start` entering lo
    auto chain = [&](uint32_t start, uint32_t lo, uint32_t hi, bool all) {
        std::vector<uint32_t> r{start};
        uint32_t cur = start;
        for (uint32_t o = lo; o < hi;) {
            if (pairs && o + 1 < hi) {
                if (all) r.push_back(c.pbs(c.lin({{cur, 1}, {g_at(o), (int32_t)mm}}), step));
                cur = c.pbs(c.lin({{cur, 1}, {g_at(o), (int32_t)mm}, {g_at(o + 1), (int32_t)W}}), step2);
                o += 2;
            } else {
                cur = c.pbs(c.lin({{cur, 1}, {g_at(o), (int32_t)mm}}), step);
                o += 1;
            }
            if (all) r.push_back(cur);
        }
        if (!all) r.assign(1, cur);
        return r;
    };
    uint32_t B = 1;
    while ((pairs ? 1ull : 2ull) * B * B < n_ext) B++;        // minimises (2 B or B) + n / B
    if (p_large()) B = std::max(B, std::min<uint32_t>(64, n_ext));      // N >= 16384: a level costs what its lookups cost, fewer hypotheses' worth of them
    const uint32_t nb = (n_ext + B - 1) / B;
    std::vector<uint32_t> r_true(n_ext + 1);
    {
        const std::vector<uint32_t> r0 = chain(zero, 0, std::min(B, n_ext), true);
        std::copy(r0.begin(), r0.end(), r_true.begin());
    }
    uint32_t R = r_true[std::min(B, n_ext)];                  // true state entering block 1
    for (uint32_t b = 1; b < nb; b++) {
        const uint32_t lo = b * B, hi = std::min(n_ext, lo + B);
        const std::vector<uint32_t> rt = chain(R, lo, hi, true);
        std::copy(rt.begin(), rt.end(), r_true.begin() + lo);
        if (b + 1 < nb) {                                      // the block's state map, then the hop to the next block
            std::vector<Term> parts;
            for (uint32_t sidx = 0; sidx < m; sidx++) {
                const uint32_t f = chain(c.trivial(sidx), lo, hi, false).back();
                const uint32_t pick = c.lut_fn([mm, sidx](uint64_t x) { return x % mm == sidx ? x / mm : (uint64_t)0; });
                parts.push_back({c.pbs(c.lin({{R, 1}, {f, (int32_t)mm}}), pick), 1});
            }
            R = c.lin(parts, 0, m - 1);                        // exactly one hypothesis is the true one
        }
    }
    const uint32_t is_sel = lut_equals(mm), nzl = lut_nonzero();
    oc.sel.resize(n);
    oc.cover.assign(n_chars, zero);
    for (uint32_t i = 0; i < n_ext; i++) {
        Scope sc(c, owner_for(i, n_ext));
        if (i < n) {
            const uint32_t x = c.lin({{r_true[i], 1}, {match[i], (int32_t)mm}});
            oc.sel[i] = i == 0 ? match[0] : c.pbs(x, is_sel);
            oc.cover[i] = i == 0 ? match[0] : c.pbs(x, nzl);
        } else {
            oc.cover[i] = c.pbs(r_true[i], nzl);
        }
    }
    return true;
}
uint32_t RunCover::running_bit(uint32_t o, uint32_t j) {
    if (!nzf || j == 0) return sel[o];
    auto key = std::make_pair(o, j);
    auto it = running.find(key);
    if (it == running.end()) it = running.emplace(key, ops.and_bits(sel[o], (*nzf)[j])).first;
    return it->second;
}
// cover[i] = [character i lies inside a selected occurrence], forward from the selection whatever produced it (the
// recurrence below, a selection taken from the right, a selection cut after n occurrences)
std::vector<uint32_t> RunCover::cover(uint32_t m, uint32_t n_chars) {
    std::vector<uint32_t> cover(n_chars);
    for (uint32_t i = 0; i < n_chars; i++) {
        std::vector<Term> terms;
        for (uint32_t j = 0; j < m && j <= i; j++)
            if (i - j < sel.size()) terms.push_back({running_bit(i - j, j), 1});
        cover[i] = ops.c.lin(terms, 0, 1);                                 // at most one occurrence covers i
        if (terms.size() > 8) cover[i] = ops.c.pbs(cover[i], ops.lut_nonzero());
    }
    return cover;
}
std::vector<uint32_t> StrOps::cover_from_sel(const std::vector<uint32_t>& sel, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf) {
    return RunCover{*this, sel, nzf, {}}.cover(m, n_chars);
}
Occurrences StrOps::occurrences(const std::vector<uint32_t>& match, uint32_t m, uint32_t n_chars, bool may_overlap,
                                const std::vector<uint32_t>* nzf) {
    Occurrences oc;
    if (may_overlap && occurrences_scan(match, m, n_chars, nzf, oc)) return oc;
    RunCover runs{*this, oc.sel, nzf, {}};              // the running bits are shared by the recurrence and the cover
    oc.sel.resize(match.size());
    const uint32_t l3 = lut_equals(3);
    // Two offsets per lookup level (default plans).  sel[o+1] needs sel[o], but sel[o] = match[o] AND NOT B with
    // B = [an earlier occurrence still runs at o], so with p = match[o] AND [the pattern is longer than one character]
    // (off the chain) and B' = [an earlier occurrence still runs at o + 1] (B' <= B: the same occurrence, one character on):
    //   sel[o+1] = match[o+1] AND NOT (p AND NOT B) AND NOT B',   one lookup on  (B + B') + 3 p + 6 match[o+1]  in [0, 11]
    // at the same level as sel[o].  Halves the depth of the recurrence (one level per TWO offsets).
    const uint32_t l_second = c.lut_fn([](uint64_t x) {
        const uint64_t mt = x / 6, pp = (x % 6) / 3, t = x % 3;
        return (uint64_t)(mt == 1 && !(pp == 1 && t == 0) && t != 2);
    });
    for (uint32_t o = 0; o < match.size(); o++) {
        std::vector<uint32_t> blockers;
        if (may_overlap)
            for (uint32_t j = 1; j < m && j <= o; j++) blockers.push_back(runs.running_bit(o - j, j));
        if (blockers.empty()) { oc.sel[o] = match[o]; continue; }
        // x = 2 match + 1 - (blockers; at most one is set) in {0..3}; selected iff x == 3
        double nu = 4 * c.node(match[o]).noise;
        for (uint32_t b : blockers) nu += c.node(b).noise;
        const bool reduced = nu > budget();
        if (reduced) blockers.assign(1, reduce_local(blockers, false));
        std::vector<Term> terms{{match[o], 2}};
        for (uint32_t b : blockers) terms.push_back({b, -1});
        oc.sel[o] = c.pbs(c.lin(terms, 1, 3), l3);
        if (!full_box_reduce || reduced || o + 1 >= match.size() || T < 12) continue;
        // the second offset of the pair, from what was known before sel[o]
        std::vector<Term> tt;
        double nu2 = 36 * c.node(match[o + 1]).noise;
        for (uint32_t b : blockers) { tt.push_back({b, 1}); nu2 += c.node(b).noise; }
        for (uint32_t j = 2; j < m && j <= o + 1; j++) {
            const uint32_t b = runs.running_bit(o + 1 - j, j);
            tt.push_back({b, 1});
            nu2 += c.node(b).noise;
        }
        const uint32_t p_bit = nzf ? and_bits(match[o], (*nzf)[1]) : match[o];
        nu2 += 9 * c.node(p_bit).noise;
        if (nu2 > budget()) continue;
        tt.push_back({p_bit, 3});
        tt.push_back({match[o + 1], 6});
        oc.sel[o + 1] = c.pbs(c.lin(tt, 0, 11), l_second);
        o++;
    }
    oc.cover = runs.cover(m, n_chars);
    return oc;
}
Str StrOps::replace_in_place(const Str& s, const Occurrences& oc, uint32_t m, const Operand& to) {
    Str out = blank(s.cap);
    for (uint32_t i = 0; i < s.cap; i++) {
        Scope sc(c, owner_for(i, s.cap));
        if (is_trivial(oc.cover[i])) { out.ch[i] = s.ch[i]; continue; }
        for (uint32_t k = 0; k < bpc; k++) {
            std::vector<Term> terms{{gate_block(s.ch[i][k], oc.cover[i], false), 1}};
            std::vector<Term> lin_contrib;      // clear `to`: v_j * sel[i - j], cheap while its noise fits
            double nu = c.node(terms[0].node).noise;
            for (uint32_t j = 0; j < m && j <= i; j++) {
                if (i - j >= oc.sel.size()) continue;
                if (to.clear()) {
                    const uint32_t v = clear_block(to.bytes[j], k);
                    if (v) { lin_contrib.push_back({oc.sel[i - j], (int32_t)v}); nu += (double)v * v * c.node(oc.sel[i - j]).noise; }
                } else {
                    terms.push_back({gate_block(to.enc->ch[j][k], oc.sel[i - j], true), 1});
                }
            }
            if (nu <= budget()) terms.insert(terms.end(), lin_contrib.begin(), lin_contrib.end());
            else for (const Term& t : lin_contrib) terms.push_back({scale_bit(t.node, (uint32_t)t.coeff), 1});
            out.ch[i].push_back(c.lin(terms, 0, M - 1));   // at most one contribution is non-zero
        }
    }
    return out;
}
// Any lengths (clear or encrypted, padded or not): every position becomes a small left-justified
// piece -- the replacement if an occurrence is selected there, the character itself if it is kept,
// nothing if it is covered -- and the pieces are concatenated pairwise (log2 n rounds of the
// occupancy-driven barrel shifter).  Result capacity = s.cap * max(1, |to| capacity), cut / padded
// to out_cap.
Str StrOps::replace_general(const Str& s, const Occurrences& oc, const Operand& to, uint32_t out_cap) {
    const uint32_t w = std::max<uint32_t>(1, to.cap());
    const uint32_t zero = c.trivial(0);
    std::vector<uint32_t> nzt;
    if (to.enc) for (uint32_t j = 0; j < to.enc->cap; j++) nzt.push_back(not_bit(char_is_zero(to.enc->ch[j])));
    const uint32_t l2 = lut_equals(2);
    std::vector<Str> cur;
    for (uint32_t i = 0; i < s.cap; i++) {
        Scope sc(c, owner_for(i, s.cap));
        const bool has_sel = i < oc.sel.size();
        const uint32_t nz = not_bit(char_is_zero(s.ch[i]));
        // kept = this slot holds a character that survives: s[i] != 0 and not covered (nz - cover + 1 == 2: and_bits would
        // take one more node for NOT cover and drops out on other constants than the test here)
        const uint32_t kept = is_trivial(oc.cover[i]) ? nz : c.pbs(c.lin({{nz, 1}, {oc.cover[i], -1}}, 1), l2);
        Str piece = blank(w, true);
        for (uint32_t j = 0; j < w; j++) {
            const bool to_slot = has_sel && j < to.cap();
            for (uint32_t k = 0; k < bpc; k++) {
                uint32_t contrib = zero;
                if (to_slot) contrib = to.enc ? gate_block(to.enc->ch[j][k], oc.sel[i], true)
                                              : scale_bit(oc.sel[i], clear_block(to.bytes[j], k));
                if (j == 0) piece.ch[j].push_back(c.lin({{gate_block(s.ch[i][k], oc.cover[i], false), 1}, {contrib, 1}}, 0, M - 1));
                else piece.ch[j].push_back(contrib);
            }
            const uint32_t sel_occ = !to_slot ? zero : (to.enc ? and_bits(oc.sel[i], nzt[j]) : oc.sel[i]);
            piece.occ[j] = j == 0 ? c.lin({{kept, 1}, {sel_occ, 1}}, 0, 1) : sel_occ;
        }
        cur.push_back(piece);
    }
    return fit(concat_tree(cur), out_cap);
}
// Empty clear pattern (Rust's str::replace("", to) / bytes.replace(b"", to)): `to` before every
// character and after the last one.
Str StrOps::replace_empty_pattern(const Str& s, const uint8_t* to_clear, uint32_t t, uint32_t out_cap) {
    if (t == 0) return fit(s, out_cap);
    const uint32_t one = c.trivial(1);
    std::vector<uint32_t> nz;
    for (uint32_t i = 0; i < s.cap; i++) nz.push_back(not_bit(char_is_zero(s.ch[i])));
    std::vector<Str> cur;
    for (uint32_t i = 0; i <= s.cap; i++) {
        Scope sc(c, owner_for(std::min(i, s.cap - 1), s.cap));
        const uint32_t g = i == 0 ? one : nz[i - 1];       // position i is still inside (or right after) the string
        Str piece = blank(t + (i < s.cap ? 1 : 0), true);
        for (uint32_t j = 0; j < t; j++) {
            for (uint32_t k = 0; k < bpc; k++) piece.ch[j].push_back(scale_bit(g, clear_block(to_clear[j], k)));
            piece.occ[j] = g;
        }
        if (i < s.cap) { piece.ch[t] = s.ch[i]; piece.occ[t] = nz[i]; }
        cur.push_back(piece);
    }
    return fit(concat_tree(cur), out_cap);
}
bool StrOps::has_border(const uint8_t* p, uint32_t m) {
    for (uint32_t b = 1; b < m; b++)
        if (std::memcmp(p, p + m - b, b) == 0) return true;
    return false;
}
void StrOps::keep_first_occurrences(Occurrences& oc, uint32_t n, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf) {
    if (n >= oc.sel.size()) return;
    const auto ge = count_ge(oc.sel, n + 1);
    for (uint32_t o = 0; o < oc.sel.size(); o++) {
        Scope sc(c, owner_for(o, (uint32_t)oc.sel.size()));
        oc.sel[o] = and_bits(oc.sel[o], not_bit(ge[n][o]));
    }
    oc.cover = cover_from_sel(oc.sel, m, n_chars, nzf);
}
// replacen with an encrypted n (thermometer g, n_max entries): a selected occurrence stays iff its running count q
// (1-based) has g_q set -- [cF[o] == q] = ge_q - ge_{q+1}, exactly one q for a selected o, none beyond n_max
void StrOps::keep_counted_occurrences(Occurrences& oc, const std::vector<uint32_t>& g, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf) {
    const uint32_t n_max = (uint32_t)g.size();
    const auto ge = count_ge(oc.sel, n_max + 1);
    const uint32_t l2 = lut_equals(2);
    for (uint32_t o = 0; o < oc.sel.size(); o++) {
        Scope sc(c, owner_for(o, (uint32_t)oc.sel.size()));
        int64_t v = 0;
        if (is_trivial(oc.sel[o], &v) && v == 0) continue;
        std::vector<Term> allowed;
        for (uint32_t q = 1; q <= n_max; q++) {
            const uint32_t hit = and_bits(c.lin({{ge[q - 1][o], 1}, {ge[q][o], -1}}, 0, 1), g[q - 1]);
            if (!(is_trivial(hit, &v) && v == 0)) allowed.push_back({hit, 1});
        }
        if (allowed.empty()) { oc.sel[o] = c.trivial(0); continue; }
        // sel + (at most one product set) == 2; a sum too noisy for one lookup is OR-ed first
        std::vector<Term> both(allowed);
        both.push_back({oc.sel[o], 1});
        const uint32_t x = c.lin(both, 0, 2);
        if (c.node(x).noise <= budget()) { oc.sel[o] = c.pbs(x, l2); continue; }
        std::vector<uint32_t> bits;
        for (const Term& t : allowed) bits.push_back(t.node);
        oc.sel[o] = and_bits(oc.sel[o], reduce_local(bits, false));
    }
    oc.cover = cover_from_sel(oc.sel, m, n_chars, nzf);
}

}  // namespace fhe
