// str_match.cpp -- StrOps: equality and order, window matching, the OR-scans, find, affix tests and strips (str_ops.h).
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <tuple>

#include "str_ops.h"

namespace fhe {

// ---- whole-string equality ----
uint32_t StrOps::eq(const Str& a, const Operand& b, bool want_equal) {
    std::vector<uint32_t> bits;
    if (b.clear()) {
        for (uint32_t i = a.cap; i < b.len; i++)
            if (b.bytes[i] != 0) return c.trivial(want_equal ? 0 : 1);   // longer than the capacity
        for (uint32_t i = 0; i < a.cap; i++) {
            Scope sc(c, owner_for(i, a.cap));
            append(bits, char_scalar_bits(a.ch[i], i < b.len ? b.bytes[i] : 0, want_equal));
        }
        return want_equal ? all_true(bits) : any_true(bits);
    }
    if (packed_compare && !want_equal) return not_bit(eq(a, b, true));   // ne = 1 - eq (linear)
    const uint32_t n = std::max(a.cap, b.enc->cap);
    for (uint32_t i = 0; i < n; i++) {
        Scope sc(c, owner_for(i, n));   // a contiguous slice of the characters per rank
        const auto* x = ch_or_null(a, i);
        const auto* y = ch_or_null(*b.enc, i);
        if (x && y) {
            if (packed_compare) append(bits, char_eq_bits(*x, *y));
            else for (uint32_t k = 0; k < bpc; k++) bits.push_back(block_eq((*x)[k], (*y)[k], want_equal));
        } else {
            // the shorter string is implicitly zero padded: compare the other one's char with 0
            append(bits, char_scalar_bits(x ? *x : *y, 0, want_equal));
        }
    }
    return want_equal ? all_true(bits) : any_true(bits);
}
// ---- pattern matching with an encrypted, zero padded pattern ----
// Several pattern characters per lookup (padding_wildcard only; relies on the padding being at the END of the pattern,
// z[i] <= z[i+1]).  With a_j in [0, n] the number of equal block (pair)s of character j and z_j its padding bit, the
// characters of a group match iff  L = sum_j (c_j a_j + d_j z_j) >= theta = n sum_j c_j  when the weights grow from the
// last character backwards as  d_j = n c_j  (a padding character counts as a full match whatever its a_j) and
// c_j = 1 + sum_{j' > j} d_j'  (one missing bit of a live character cannot be made up by everything behind it).
// L_max = 2 n sum c_j must fit [0, T]: PARAM_MESSAGE_2_CARRY_2 (n = 2 packed pairs per character): two characters,
// c = (3, 1), d = (6, 2), L in [0, 16] = the whole box incl. the padding bit (Circuit::pbs_box), 60 nominal variances.
// Halves the per-(offset, character) level of contains / find / starts_with.
GroupWeights StrOps::group_weights(uint32_t k, uint32_t n) const {
    GroupWeights w;
    w.c.assign(k, 0); w.d.assign(k, 0);
    int64_t behind = 0, csum = 0;
    for (int j = (int)k - 1; j >= 0; j--) {
        w.c[j] = (int32_t)(1 + behind);
        w.d[j] = (int32_t)(n * w.c[j]);
        behind += w.d[j];
        csum += w.c[j];
        w.noise += (double)w.c[j] * w.c[j] * n + (double)w.d[j] * w.d[j];
    }
    w.theta = (int64_t)n * csum;
    w.lmax = 2 * (int64_t)n * csum;
    return w;
}
uint32_t StrOps::group_size(uint32_t n, uint32_t remaining) const {
    uint32_t k = 1;
    while (k < remaining && k < 8) {
        const GroupWeights w = group_weights(k + 1, n);
        if (w.lmax > (int64_t)T || w.noise > budget()) break;
        k++;
    }
    return k;
}
namespace {
using Pair = std::pair<uint32_t, uint32_t>;
// The lookups of one window_matches call per (character, pattern character), each built once.
struct WindowMatcher {
    StrOps& ops;
    Circuit& c;
    const Str &s, &pat;
    std::vector<uint32_t> z;                                        // z[i] = [pat[i] == 0]
    std::map<Pair, Pair> sums;
    std::map<Pair, uint32_t> chars;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> groups;
    std::map<uint32_t, uint32_t> s_zero;
    WindowMatcher(StrOps& ops, const Str& s, const Str& pat) : ops(ops), c(ops.c), s(s), pat(pat) {
        for (uint32_t i = 0; i < pat.cap; i++) z.push_back(ops.char_is_zero(pat.ch[i]));
    }
    // sum of the block-equality bits of (s[ci], pat[pi]) and how many bits that is (n: all equal)
    Pair char_eq_sum(uint32_t ci, uint32_t pi) {
        auto it = sums.find({ci, pi});
        if (it != sums.end()) return it->second;
        const std::vector<uint32_t> bits = ops.char_eq_bits(s.ch[ci], pat.ch[pi]);
        std::vector<Term> terms;
        for (uint32_t bit : bits) terms.push_back({bit, 1});
        return sums[{ci, pi}] = Pair(c.lin(terms), (uint32_t)bits.size());
    }
    // padding_wildcard: [pat[pi] == 0] OR [s[ci] == pat[pi]]  (prefix-style match: pattern padding matches anything)
    // otherwise:        [s[ci] == pat[pi]]                    (exact match incl. padding)
    uint32_t char_match(uint32_t ci, uint32_t pi, bool padding_wildcard) {
        if (ci >= s.cap) return z[pi];   // null char: equal iff pat[pi] == 0 (both readings)
        auto it = chars.find({ci, pi});
        if (it != chars.end()) return it->second;
        const Pair sn = char_eq_sum(ci, pi);
        const uint32_t sum = sn.first, n = sn.second;
        // wildcard: value = eq_sum + n*z in [0, 2n]  ->  match iff value >= n (z = 1, or all n bits set)
        return chars[{ci, pi}] = padding_wildcard
            ? c.pbs(c.lin({{sum, 1}, {z[pi], (int32_t)n}}), c.lut_fn([n](uint64_t x) { return (uint64_t)(x >= n); }))
            : c.pbs(sum, ops.lut_equals(n));
    }
    // k pattern characters from pi on against the characters from ci on, in one lookup (the weights: group_weights)
    uint32_t group_match(uint32_t ci, uint32_t pi, uint32_t k) {
        if (ci >= s.cap) return z[pi];          // the whole group lies behind the string: all of it must be padding = z[pi]
        auto key = std::make_tuple(ci, pi, k);
        auto it = groups.find(key);
        if (it != groups.end()) return it->second;
        uint32_t n = 0;
        std::vector<uint32_t> a(k, UINT32_MAX);
        for (uint32_t j = 0; j < k; j++) {
            if (ci + j >= s.cap) continue;      // behind the string: no equal blocks, only its padding bit can save it
            const Pair sn = char_eq_sum(ci + j, pi + j);
            a[j] = sn.first;
            n = sn.second;
        }
        const GroupWeights w = ops.group_weights(k, n);
        std::vector<Term> terms;
        for (uint32_t j = 0; j < k; j++) {
            if (a[j] != UINT32_MAX) terms.push_back({a[j], w.c[j]});
            terms.push_back({z[pi + j], w.d[j]});
        }
        const uint32_t L = c.lin(terms);
        const int64_t theta = w.theta;
        if (c.node(L).vmax >= (int64_t)ops.T) {
            std::vector<uint8_t> g(ops.T);
            for (uint32_t x = 0; x < ops.T; x++) g[x] = (int64_t)x >= theta;
            return groups[key] = c.pbs_box(L, g);
        }
        return groups[key] = c.pbs(L, c.lut_fn([theta](uint64_t x) { return (uint64_t)((int64_t)x >= theta); }));
    }
    uint32_t end_bit(uint32_t ci) {             // [s[ci] == 0]
        auto it = s_zero.find(ci);
        return it != s_zero.end() ? it->second : s_zero[ci] = ops.char_is_zero(s.ch[ci]);
    }
};
}  // namespace
std::vector<uint32_t> StrOps::window_matches(const Str& s, const Str& pat, uint32_t n_off, bool padding_wildcard, bool need_end) {
    WindowMatcher w(*this, s, pat);
    // characters per lookup: more than one only with wildcard padding, in the default (not reference-shaped) plans
    uint32_t per_lookup = 1;
    if (padding_wildcard && full_box_reduce && pat.cap > 1 && s.cap > 0) {
        // how many equality bits a character has ((s[0], pat[0]) is needed by offset 0 anyway; memoised in `sums`)
        per_lookup = group_size(w.char_eq_sum(0, 0).second, pat.cap);
    }
    std::vector<uint32_t> match;
    for (uint32_t o = 0; o < n_off; o++) {
        Scope sc(c, owner_for(o, n_off));   // a contiguous slice of the offsets per rank
        std::vector<uint32_t> bits;
        if (per_lookup > 1) {
            for (uint32_t i = 0; i < pat.cap; i += per_lookup)
                bits.push_back(w.group_match(o + i, i, std::min(per_lookup, pat.cap - i)));
        } else if (!padding_wildcard && full_box_reduce) {
            // exact match incl. padding: no per-character lookup at all -- the equal-block counts of up to T / n
            // characters are summed and tested against their maximum in one lookup (T itself through pbs_full_box)
            std::vector<Term> run;
            int64_t run_max = 0;
            auto flush = [&]() {
                if (run.empty()) return;
                const uint32_t sum = c.lin(run);
                bits.push_back(run_max == (int64_t)T ? c.pbs_full_box(sum, true) : c.pbs(sum, lut_equals((uint64_t)run_max)));
                run.clear();
                run_max = 0;
            };
            for (uint32_t i = 0; i < pat.cap; i++) {
                if (o + i >= s.cap) { bits.push_back(w.z[i]); continue; }       // behind the string: the pattern must be padding there
                const auto sn = w.char_eq_sum(o + i, i);
                if (run_max + (int64_t)sn.second > (int64_t)T || c.node(sn.first).noise * (double)(run.size() + 1) > budget()) flush();
                run.push_back({sn.first, 1});
                run_max += sn.second;
            }
            flush();
        } else {
            for (uint32_t i = 0; i < pat.cap; i++) bits.push_back(w.char_match(o + i, i, padding_wildcard));
        }
        if (need_end && o + pat.cap < s.cap) bits.push_back(w.end_bit(o + pat.cap));
        match.push_back(all_true(bits));
    }
    return match;
}
// Clear pattern, whole characters as lookup inputs (4-bit blocks, 8-bit plaintext space): classify instead of
// compare.  Level 1 maps every character to the id of the distinct pattern character it equals (0 = none), one
// PBS per position whatever the pattern; level L = 2, 4, ... maps the pair (class of the window of length L/2 at t,
// class of the one at t + L/2), packed as a + B b, to the id of the pattern substring of length L it spells
// (0 = none).  A window equals at most one distinct substring, so ids are well defined even with repeated
// characters.  match[o] is the class of the whole pattern at o (two overlapping top windows and one more PBS
// when len is not a power of two).  Cost: about (1 + log2 len) PBS per position instead of (distinct characters
// + AND tree): 3,068 instead of 5,105 for a 4-char pattern in 1024 chars, 5 n instead of ~18 n for 16 chars.
// Returns false when a packing does not fit (space or noise budget): the caller falls back.
bool StrOps::window_matches_clear_classes(const Str& s, const uint8_t* pat, uint32_t len, uint32_t n_off, std::vector<uint32_t>& match) {
    if (len < 2 || n_off < 2) return false;
    const uint32_t span = n_off + len - 1;                 // characters any window touches
    for (uint32_t t = 0; t < span; t++) if (!whole_char_fits(s.ch[t])) return false;
    uint32_t top = 1;
    while (top * 2 <= len) top *= 2;
    // offsets (inside the pattern) of the windows needed at every length
    std::map<uint32_t, std::set<uint32_t>> need;
    need[top].insert(0);
    if (top != len) need[top].insert(len - top);
    for (uint32_t L = top; L >= 2; L /= 2)
        for (uint32_t o : need[L]) { need[L / 2].insert(o); need[L / 2].insert(o + L / 2); }
    // ids of the distinct needed substrings per length
    std::map<uint32_t, std::map<std::string, uint32_t>> ids;
    for (auto& [L, offs] : need)
        for (uint32_t o : offs) {
            const std::string sub(reinterpret_cast<const char*>(pat) + o, L);
            if (!ids[L].count(sub)) { const uint32_t id = (uint32_t)ids[L].size() + 1; ids[L][sub] = id; }
        }
    for (uint32_t L = 1; L < top; L *= 2) {
        const uint64_t B = ids[L].size() + 1;
        if (B * B > T || 1.0 + (double)(B * B) > budget()) return false;      // pbs outputs are nominal: 1 + B^2 variances
    }
    if (top != len) { const uint64_t B = ids[top].size() + 1; if (B * B > T || 1.0 + (double)(B * B) > budget()) return false; }
    // level 1
    std::vector<uint32_t> cur(span);
    {
        std::vector<uint64_t> table(256, 0);
        for (auto& [sub, id] : ids[1]) table[(uint8_t)sub[0]] = id;
        const uint32_t l1 = c.lut_fn([&](uint64_t x) { return x < 256 ? table[x] : 0; });
        for (uint32_t t = 0; t < span; t++) {
            Scope sc(c, owner_for(t, span));
            cur[t] = c.pbs(whole_char(s.ch[t]), l1);
        }
    }
    // doubling
    for (uint32_t L = 2; L <= top; L *= 2) {
        const uint32_t B = (uint32_t)ids[L / 2].size() + 1, count = span - L + 1;
        std::map<uint64_t, uint64_t> pair_id;           // a + B b -> id
        for (auto& [sub, id] : ids[L])
            pair_id[ids[L / 2].at(sub.substr(0, L / 2)) + (uint64_t)B * ids[L / 2].at(sub.substr(L / 2))] = id;
        const uint32_t lut = c.lut_fn([&](uint64_t x) { auto it = pair_id.find(x); return it == pair_id.end() ? (uint64_t)0 : it->second; });
        std::vector<uint32_t> next(count);
        for (uint32_t t = 0; t < count; t++) {
            Scope sc(c, owner_for(t, count));
            next[t] = c.pbs(c.lin({{cur[t], 1}, {cur[t + L / 2], (int32_t)B}}), lut);
        }
        cur.swap(next);
    }
    match.clear();
    if (top == len) {            // one class at the top: its id 1 is the match bit
        match.assign(cur.begin(), cur.begin() + n_off);
        return true;
    }
    const uint32_t B = (uint32_t)ids[top].size() + 1;
    const uint64_t want = ids[top].at(std::string(reinterpret_cast<const char*>(pat), top)) +
                          (uint64_t)B * ids[top].at(std::string(reinterpret_cast<const char*>(pat) + len - top, top));
    const uint32_t fin = lut_equals(want);
    for (uint32_t o = 0; o < n_off; o++) {
        Scope sc(c, owner_for(o, n_off));
        match.push_back(c.pbs(c.lin({{cur[o], 1}, {cur[o + len - top], (int32_t)B}}), fin));
    }
    return true;
}
std::vector<uint32_t> StrOps::window_matches_clear(const Str& s, const uint8_t* pat, uint32_t len, uint32_t n_off) {
    {
        std::vector<uint32_t> classed;
        if (window_matches_clear_classes(s, pat, len, n_off, classed)) return classed;
    }
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> memo;   // (char, byte) -> bits
    std::vector<uint32_t> match;
    for (uint32_t o = 0; o < n_off; o++) {
        Scope sc(c, owner_for(o, n_off));
        std::vector<uint32_t> bits;
        for (uint32_t i = 0; i < len; i++) {
            auto key = std::make_pair(o + i, (uint32_t)pat[i]);
            auto it = memo.find(key);
            if (it == memo.end()) it = memo.emplace(key, char_scalar_bits(s.ch[o + i], pat[i], true)).first;
            append(bits, it->second);
        }
        match.push_back(all_true(bits));
    }
    return match;
}
// (o + len == cap or s[o + len] == 0; the lookup is spelled out: in a program the end test may be known at build time, where and_bits would drop out)
std::vector<uint32_t> StrOps::ending_here(const Str& s, const std::vector<uint32_t>& match, uint32_t len) {
    std::vector<uint32_t> cand;
    for (uint32_t o = 0; o + len < s.cap; o++) {
        const uint32_t zend = char_is_zero(s.ch[o + len]);
        cand.push_back(c.pbs(c.lin({{match[o], 1}, {zend, 1}}), lut_equals(2)));
    }
    cand.push_back(match[s.cap - len]);
    return cand;
}
uint32_t StrOps::starts_with(const Str& s, const Operand& pat) {
    if (!pat.clear()) return window_matches(s, *pat.enc, 1, true)[0];
    if (pat.len > s.cap) return c.trivial(0);
    if (pat.len == 0) return c.trivial(1);
    return window_matches_clear(s, pat.bytes, pat.len, 1)[0];
}
uint32_t StrOps::contains(const Str& s, const Operand& pat) {
    if (!pat.clear()) return any_true(window_matches(s, *pat.enc, s.cap, true));
    if (pat.len > s.cap) return c.trivial(0);
    if (pat.len == 0) return c.trivial(1);
    return any_true(window_matches_clear(s, pat.bytes, pat.len, s.cap - pat.len + 1));
}
// ends_with: some suffix of s (incl. the empty one at offset cap) equals the whole padded pattern
uint32_t StrOps::ends_with(const Str& s, const Operand& pat) {
    if (!pat.clear()) return any_true(window_matches(s, *pat.enc, s.cap + 1, false, true));
    if (pat.len > s.cap) return c.trivial(0);
    if (pat.len == 0) return c.trivial(1);
    return any_true(ending_here(s, window_matches_clear(s, pat.bytes, pat.len, s.cap - pat.len + 1), pat.len));
}
// ---- find: (found, index digits) of the first match ----
// The core of the blocked OR-scans: runs of scan_run() bits, each scanned on its own (fan-in up to T per PBS).
StrOps::RunScan StrOps::scan_runs(const std::vector<uint32_t>& bits) {
    const uint32_t F = scan_run(), nz = lut_nonzero();
    const size_t n = bits.size();
    RunScan scan;
    scan.within.resize(n);
    for (size_t b = 0; b < n; b += F) {
        std::vector<Term> run;
        for (size_t j = b; j < std::min(n, b + F); j++) {
            run.push_back({bits[j], 1});
            scan.within[j] = run.size() == 1 ? bits[j] : run.size() == T ? c.pbs_full_box(c.lin(run), false) : c.pbs(c.lin(run), nz);
        }
        scan.tot.push_back(scan.within[std::min(n, b + F) - 1]);
    }
    return scan;
}
// prefix_any[o] = OR_{o' <= o} bits[o'] through a blocked scan
std::vector<uint32_t> StrOps::prefix_or(const std::vector<uint32_t>& bits_in) {
    const uint32_t F = scan_run(), nz = lut_nonzero();     // (the table is numbered here, used or not)
    const size_t n = bits_in.size();
    if (n <= 1) return bits_in;
    // a block whose bits are sums over shared lookup outputs may pass the noise budget as a run (sum_noise: rsplit,
    // rsplitn and rsplit_once with a clear pattern of 6 characters and more reached 106 .. 122 nominal variances and
    // were refused): its bits get a lookup of their own first.  A plan whose runs fit is built exactly as before.
    std::vector<uint32_t> bits(bits_in);
    for (size_t b = 0; b < n; b += F) {
        std::vector<Term> block;
        for (size_t j = b; j < std::min(n, b + F); j++) block.push_back({bits[j], 1});
        if (sum_noise(block) <= budget()) continue;
        const uint32_t is_one = lut_equals(1);
        for (size_t j = b; j < std::min(n, b + F); j++)
            if (c.node(bits[j]).noise > 1.0) bits[j] = c.pbs(bits[j], is_one);
    }
    const RunScan scan = scan_runs(bits);
    if (scan.tot.size() == 1) return scan.within;
    std::vector<uint32_t> block_pre = prefix_or(scan.tot);   // inclusive prefix over blocks
    std::vector<uint32_t> out(n);
    for (size_t j = 0; j < n; j++) {
        const size_t b = j / F;
        out[j] = b == 0 ? scan.within[j] : c.pbs(c.lin({{scan.within[j], 1}, {block_pre[b - 1], 1}}), nz);
    }
    return out;
}
std::vector<uint32_t> StrOps::find_from_matches(const std::vector<uint32_t>& match_in, uint32_t n_digits, bool from_end) {
    std::vector<uint32_t> match(match_in);
    if (from_end) std::reverse(match.begin(), match.end());
    // first[o] = match[o] AND no match before o.  "Before o" = earlier in o's block of the scan (prefix inside the
    // block) or in an earlier block (prefix over the block totals): the two are fed to the lookup side by side,
    // (match[o] + 2 * before_in_block + 4 * before_in_earlier_blocks) == 1, so the full prefix is never materialised
    // (one lookup level and n lookups less than prefix_or + a test against it).
    const uint32_t first_lut = lut_equals(1), nz = lut_nonzero(), Fb = scan_run();
    const size_t n = match.size();
    if (n == 0) {                                   // no candidate offset at all: not found, index 0 (a constant of its own each)
        std::vector<uint32_t> none;
        for (uint32_t d = 0; d < 1 + n_digits; d++) none.push_back(c.trivial(0));
        return none;
    }
    const RunScan scan = scan_runs(match);
    const std::vector<uint32_t>& within = scan.within;
    const std::vector<uint32_t> block_pre = prefix_or(scan.tot);       // inclusive, over the blocks
    std::vector<uint32_t> first(n);
    for (size_t o = 0; o < n; o++) {
        const size_t b = o / Fb, r = o % Fb;
        std::vector<Term> t{{match[o], 1}};
        if (T >= 8) {
            if (r > 0) t.push_back({within[o - 1], 2});
            if (b > 0) t.push_back({block_pre[b - 1], 4});
        } else if (r > 0 && b > 0) {
            // boxes of fewer than 8 values (PARAM_MESSAGE_1_CARRY_1: T = 4) cannot hold the three bits side by side
            // (ADVICE r3): the two "before" bits are OR-ed by one more lookup, then match + 2 * before <= 3
            t.push_back({c.pbs(c.lin({{within[o - 1], 1}, {block_pre[b - 1], 1}}), nz), 2});
        } else if (r > 0) {
            t.push_back({within[o - 1], 2});
        } else if (b > 0) {
            t.push_back({block_pre[b - 1], 2});
        }
        first[o] = t.size() == 1 ? match[o] : c.pbs(c.lin(t), first_lut);
    }
    if (from_end) std::reverse(first.begin(), first.end());   // one-hot vector back on the original offsets
    std::vector<uint32_t> out{block_pre.back()};              // found
    const uint32_t F = T - 1, idm = lut_message();
    for (uint32_t d = 0; d < n_digits; d++) {
        // digit d of the index = sum_o first[o] * digit_d(o): at most one term is non-zero, so the
        // value stays <= M-1 whatever the fan-in; what limits a group is the noise, dig^2 per term
        std::vector<Term> parts;
        for (size_t o = 0; o < first.size(); o++) {
            const uint32_t dig = (uint32_t)((o >> (d * bits_per_block)) & (M - 1));
            if (dig) parts.push_back({first[o], (int32_t)dig});
        }
        std::vector<uint32_t> cleaned;
        do {                                                  // the groups' lookups are summed in turn: again at most one is non-zero
            cleaned.clear();
            for (const auto& g : term_groups(parts, F)) cleaned.push_back(c.pbs(c.lin(g, 0, (int64_t)M - 1), idm));
            parts.clear();
            for (uint32_t p : cleaned) parts.push_back({p, 1});
        } while (cleaned.size() > 1);
        out.push_back(cleaned.empty() ? c.trivial(0) : cleaned[0]);
    }
    return out;
}
std::vector<uint32_t> StrOps::prefix_or_known(const std::vector<uint32_t>& bits) {
    auto known_zero = [&](uint32_t b) { int64_t v = 0; return is_trivial(b, &v) && v == 0; };
    size_t lo = 0, hi = bits.size();
    while (lo < hi && known_zero(bits[lo])) lo++;
    while (hi > lo && known_zero(bits[hi - 1])) hi--;
    std::vector<uint32_t> out(bits.size(), c.trivial(0));
    if (lo == hi) return out;
    const std::vector<uint32_t> core = prefix_or(std::vector<uint32_t>(bits.begin() + lo, bits.begin() + hi));
    std::copy(core.begin(), core.end(), out.begin() + lo);
    for (size_t j = hi; j < bits.size(); j++) out[j] = core.back();
    return out;
}
// strip_prefix: if s starts with the pattern, drop it.  Clear pattern of length m: shift left by m.  Encrypted (padded)
// pattern: shift left by its hidden length -- the barrel shifter's monotone indicator is sel AND [pat[t] != 0]
Str StrOps::strip_prefix(const Str& s, const Operand& pat, uint32_t* stripped_bit) {
    const uint32_t sel = *stripped_bit = starts_with(s, pat);
    if (pat.clear()) {
        const uint32_t m = pat.len;
        if (m == 0 || m > s.cap) return s;
        return build_str(s.cap, [&](uint32_t i, uint32_t k) {
            return i + m < s.cap ? select_gated(sel, s.ch[i + m][k], s.ch[i][k]) : gate_block(s.ch[i][k], sel, false);
        });
    }
    std::vector<uint32_t> lead(s.cap, c.trivial(0));
    for (uint32_t t = 0; t < std::min(s.cap, pat.enc->cap); t++) lead[t] = and_bits(sel, not_bit(char_is_zero(pat.enc->ch[t])));
    return shift_left_by_leading(s, lead);
}
// strip_suffix: cand[o] = "s[o..] is exactly the pattern" (encrypted, padded pattern: window match incl. the
// end-of-string test); every character from the first such o on is zeroed
Str StrOps::strip_suffix(const Str& s, const Operand& pat, uint32_t* stripped_bit) {
    std::vector<uint32_t> cut;                              // cut[i] = the suffix starts at or before i
    if (pat.clear()) {
        if (pat.len > s.cap) { *stripped_bit = c.trivial(0); return s; }
        if (pat.len == 0) { *stripped_bit = c.trivial(1); return s; }
        const std::vector<uint32_t> m = window_matches_clear(s, pat.bytes, pat.len, s.cap - pat.len + 1);
        if (pat.len < s.cap) lut_equals(2);                 // this plan numbers the AND table ahead of the end tests' tables
        cut = prefix_or(ending_here(s, m, pat.len));
        *stripped_bit = cut.back();
    } else {
        const std::vector<uint32_t> cand = window_matches(s, *pat.enc, s.cap + 1, false, true);
        cut = prefix_or(std::vector<uint32_t>(cand.begin(), cand.begin() + s.cap));
        *stripped_bit = reduce_local({cut.back(), cand[s.cap]}, false);
    }
    return build_str(s.cap, [&](uint32_t i, uint32_t k) { return gate_block(s.ch[i][k], cut[std::min<size_t>(i, cut.size() - 1)], false); });
}
// ---- lexicographic order (the reference's comparator idea: per-block sign, then pairwise
//      selection "most significant non-equal wins", integer/server_key/comparator.rs:226-280) ----
// sign encoding: 0 = a < b, 1 = equal, 2 = a > b.  Strings compare like big-endian integers of
// their (zero padded) bytes, which is exactly bytes.__lt__ on the unpadded strings.
uint32_t StrOps::compare_sign(const Str& a, const Operand& rhs) {
    const Str* const b = rhs.enc;           // null: the clear bytes of rhs
    const uint32_t n = std::max(a.cap, rhs.cap());
    std::vector<uint32_t> signs;   // most significant first
    const uint32_t mm = M;
    for (uint32_t i = 0; i < n; i++) {
        bool packed = b && packed_compare && bpc % 2 == 0 && i < a.cap && i < b->cap;
        for (uint32_t k = 0; packed && k + 1 < bpc; k += 2)
            packed = packed_pair_fits(a.ch[i][k], a.ch[i][k + 1], b->ch[i][k], b->ch[i][k + 1]);
        if (packed) {
            // sign of a packed block pair in one PBS: the sign function is odd, hence negacyclic for
            // free -- f(0) = 0, f(1..T-1) = 1 gives -1 on the negative (padding-bit) side; +1 maps
            // {-1, 0, 1} onto the {0, 1, 2} encoding
            const uint32_t l = lut_nonzero();
            for (int k = (int)bpc - 2; k >= 0; k -= 2) {
                const uint32_t d = c.lin({{a.ch[i][k], 1}, {a.ch[i][k + 1], (int32_t)M}, {b->ch[i][k], -1},
                                          {b->ch[i][k + 1], -(int32_t)M}});
                signs.push_back(c.lin({{c.pbs(d, l, /*signed_input=*/true), 1}}, 1, 2));
            }
            continue;
        }
        for (int k = (int)bpc - 1; k >= 0; k--) {
            const bool has_a = i < a.cap;
            if (b) {
                const bool has_b = i < b->cap;
                if (has_a && has_b) {   // sign(a - b) from a - b + (M-1) in [0, 2M-2]
                    const uint32_t l = c.lut_fn([mm](uint64_t x) { return (uint64_t)(x < mm - 1 ? 0 : (x == mm - 1 ? 1 : 2)); });
                    signs.push_back(c.pbs(c.lin({{a.ch[i][k], 1}, {b->ch[i][k], -1}}, (int64_t)M - 1, 2 * ((int64_t)M - 1)), l));
                } else {               // the missing side is a null char
                    const uint32_t l = c.lut_fn([has_a](uint64_t x) { return (uint64_t)(x == 0 ? 1 : (has_a ? 2 : 0)); });
                    signs.push_back(c.pbs(has_a ? a.ch[i][k] : b->ch[i][k], l));
                }
            } else {
                const uint32_t v = clear_block(i < rhs.len ? rhs.bytes[i] : 0, (uint32_t)k);
                if (!has_a) { if (v) signs.push_back(c.trivial(0)); continue; }   // a is null there: a < clear iff clear != 0
                const uint32_t l = c.lut_fn([v](uint64_t x) { return (uint64_t)(x < v ? 0 : (x == v ? 1 : 2)); });
                signs.push_back(c.pbs(a.ch[i][k], l));
            }
        }
    }
    if (signs.empty()) return c.trivial(1);
    const uint32_t pick = c.lut_fn([](uint64_t x) { const uint64_t hi = x / 3, lo = x % 3; return hi != 1 ? (hi > 2 ? (uint64_t)1 : hi) : lo; });
    return tree_reduce(signs, [&](uint32_t hi, uint32_t lo) { return c.pbs(c.lin({{hi, 3}, {lo, 1}}, 0, 8), pick); })[0];
}
uint32_t StrOps::order_bit(uint32_t sign, const std::string& op) {
    const bool lt = op == "lt", le = op == "le", gt = op == "gt";
    const uint32_t l = c.lut_fn([lt, le, gt](uint64_t s) {
        return (uint64_t)(lt ? s == 0 : (le ? s != 2 : (gt ? s == 2 : s != 0)));
    });
    return c.pbs(sign, l);
}

}  // namespace fhe
