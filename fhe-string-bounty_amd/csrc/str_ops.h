// str_ops.h -- StrOps: the FheString operations as batched shortint circuits, one class over a Circuit.
//
// An FheString is `cap` characters, zero padded; one 8-bit character = 8/log2(msg_mod) shortint blocks, little endian
// (integer/block_decomposition.rs:119-144).  Semantics of every operation = the corresponding clear-text function on the
// unpadded ASCII string.  The members are defined in themed units, named section by section below
// (str_ops.cpp where none is named), with the algorithms described at the definitions; fhe_string.cpp holds the op
// dispatch (OpBuilder, build_string_op).
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "circuit.h"
#include "regex.h"
#include "str_op_name.h"

namespace fhe {

struct Str {
    uint32_t cap = 0;
    std::vector<std::vector<uint32_t>> ch;   // [char][block] node ids
    std::vector<uint32_t> occ;               // optional, [char]: 0/1 node "this slot holds a character"
};
// The right operand of an operation: an encrypted (zero padded) string, or `len` clear bytes.
struct Operand {
    const Str* enc = nullptr;
    const uint8_t* bytes = nullptr;     // len of them
    uint32_t len = 0;
    Operand(const Str& s) : enc(&s) {}
    Operand(const uint8_t* bytes, uint32_t len) : bytes(bytes), len(len) {}
    bool clear() const { return !enc; }
    uint32_t cap() const { return enc ? enc->cap : len; }
};
// Occurrence bookkeeping of a replace: which offsets are selected (leftmost, non-overlapping) and which characters they
// cover.  An occurrence selected at o - j still runs at o iff j < |from|: always for a clear / unpadded pattern of length
// m, and iff nzf[j] = [from[j] != 0] for a padded encrypted one (nzf == nullptr: unpadded).
struct Occurrences {
    std::vector<uint32_t> sel;     // [offset]
    std::vector<uint32_t> cover;   // [char] 0/1: inside a selected occurrence
};
struct GroupWeights { std::vector<int32_t> c, d; int64_t theta = 0, lmax = 0; double noise = 0; };   // str_match.cpp: group_match
// (offset, j) -> sel[offset] AND nzf[j]: the occurrence selected at `offset` still runs j characters on
using RunMemo = std::map<std::pair<uint32_t, uint32_t>, uint32_t>;
// Where a string is cut: a clear position n, or an encrypted one -- its digits (count_inputs) and n = the public bound n_max.
struct Position {
    uint32_t n = 0;
    const std::vector<uint32_t>* digits = nullptr;
    bool enc() const { return digits != nullptr; }
};

class StrOps {
public:
    explicit StrOps(Circuit& c) : c(c) {
        M = c.msg_modulus();
        T = c.total_modulus();
        bits_per_block = 0;
        while ((1u << bits_per_block) < M) bits_per_block++;
        bpc = 8 / bits_per_block;
        ok = (1u << bits_per_block) == M && 8 % bits_per_block == 0 && T / M >= M;
        world = c.build_world();
    }
    Circuit& c;
    uint32_t M, T, bits_per_block, bpc, world;
    bool ok;
    // Encrypted-vs-encrypted comparisons: true = compare two blocks per PBS (see packed_pair_eq),
    // false = the reference's one-bivariate-PBS-per-block shape (comparison.rs:10-33).
    bool packed_compare = true;
    bool full_box_reduce = true;       // reductions take T bits per lookup (false: T - 1, the reference's chunks)
    bool blocked_scan = true;          // occurrences: the blocked scan where it fits (occurrences_scan)
    using SplitKind = opname::SplitKind;        // which operation of the family (str_op_name.h)

    // ---- multi-GPU: which rank owns the work on element idx of `total` (contiguous slices) ----
    int owner_for(uint32_t idx, uint32_t total) const { return world > 1 && total ? (int)((uint64_t)idx * world / total) : -1; }
    struct Scope {   // PBS nodes created while alive belong to `rank` (no-op for rank < 0)
        Circuit& c; int prev;
        Scope(Circuit& c, int rank) : c(c), prev(c.owner_hint()) { if (rank >= 0) c.set_owner_hint(rank); }
        ~Scope() { c.set_owner_hint(prev); }
    };
    // ---- noise: split a sum into pieces one lookup may take (value bound max_terms, noise budget) ----
    double budget() const { return c.noise_budget() > 0 ? c.noise_budget() : 1e300; }
    bool p_large() const { return c.params().N >= 16384; }      // a lookup level costs what its lookups cost, not one PBS latency
    // A whole character as ONE lookup input, hi * M + lo: needs two blocks per char whose 8 bits fit the message +
    // carry space (PARAM_MESSAGE_4_CARRY_4: 4-bit blocks, 256 plaintexts) and 1 + M^2 nominal variances within the
    // noise budget -- "one PBS per encrypted character".  Per-character predicates and case conversion then cost 1
    // PBS instead of 3.
    bool whole_char_fits(const std::vector<uint32_t>& b) const {
        return bpc == 2 && (uint64_t)M * M <= (uint64_t)T && c.node(b[0]).noise + (double)M * M * c.node(b[1]).noise <= budget();
    }
    uint32_t whole_char(const std::vector<uint32_t>& b) { return c.lin({{b[1], (int32_t)M}, {b[0], 1}}); }
    // the noise of sum_t coeff_t * node_t as Circuit::lin will build it (shared sources add up by coefficient)
    double sum_noise(const std::vector<Term>& terms) const;
    std::vector<std::vector<Term>> term_groups(const std::vector<Term>& terms, size_t max_terms) const;
    bool is_trivial(uint32_t node, int64_t* value = nullptr) const {       // a constant known at build time (and its value)
        const Node& n = c.node(node);
        if (n.kind != Node::LIN || !n.terms.empty()) return false;
        if (value) *value = n.cst;
        return true;
    }

    // ---- strings block by block ----
    // `cap` characters without blocks yet (with_occ: and as many occupancy slots)
    Str blank(uint32_t cap, bool with_occ = false) const {
        Str s;
        s.cap = cap, s.ch.resize(cap), s.occ.resize(with_occ ? cap : 0);
        return s;
    }
    // block k of character i = f(i, k), created character by character
    template <class F>
    Str build_str(uint32_t cap, F f) {
        Str s = blank(cap);
        for (uint32_t i = 0; i < cap; i++)
            for (uint32_t k = 0; k < bpc; k++) s.ch[i].push_back(f(i, k));
        return s;
    }
    Str input_string(uint32_t cap) { return build_str(cap, [&](uint32_t, uint32_t) { return c.input(M - 1); }); }
    Str clear_string(const uint8_t* bytes, uint32_t len) { return build_str(len, [&](uint32_t i, uint32_t k) { return c.trivial(clear_block(bytes[i], k)); }); }
    uint32_t clear_block(uint8_t v, uint32_t b) const { return (v >> (b * bits_per_block)) & (M - 1); }    // clear byte -> block digits
    const std::vector<uint32_t>* ch_or_null(const Str& s, uint32_t i) const { return i < s.cap ? &s.ch[i] : nullptr; }
    Str fit(const Str& r, uint32_t cap);                    // cut or zero-pad to `cap` characters
    void emit(const Str& s) { for (auto& blocks : s.ch) for (uint32_t b : blocks) c.output(b); }   // every block an output

    // ---- the 0/1 tables used all over (a table is numbered where it is first created: callers keep their order) ----
    uint32_t lut_nonzero() { return c.lut_fn([](uint64_t x) { return (uint64_t)(x != 0); }); }
    uint32_t lut_equals(uint64_t k) { return c.lut_fn([k](uint64_t x) { return (uint64_t)(x == k); }); }
    uint32_t lut_message() { const uint32_t mm = M; return c.lut_fn([mm](uint64_t x) { return x % mm; }); }

    // ---- reductions of 0/1 blocks ----
    uint32_t reduce_local(std::vector<uint32_t> bits, bool all);           // AND / OR on one rank, chunks of up to T bits
    uint32_t reduce_bits(const std::vector<uint32_t>& bits, bool all);     // the same, every rank reducing its own bits first
    uint32_t all_true(const std::vector<uint32_t>& bits) { return reduce_bits(bits, true); }
    uint32_t any_true(const std::vector<uint32_t>& bits) { return reduce_bits(bits, false); }
    // pairwise tree reduction: neighbours are joined level by level until `until` are left; an odd last one moves up as it is
    template <class V, class F>
    std::vector<V> tree_reduce(std::vector<V> v, F join, size_t until = 1) {
        while (v.size() > until) {
            std::vector<V> next;
            for (size_t i = 0; i + 1 < v.size(); i += 2) next.push_back(join(v[i], v[i + 1]));
            if (v.size() & 1) next.push_back(v.back());
            v.swap(next);
        }
        return v;
    }
    // message_extract of a block that carries more than nominal noise: back to NoiseLevel::NOMINAL for one PBS
    std::map<uint32_t, uint32_t> fresh_memo;
    uint32_t fresh(uint32_t block);

    // ---- block-level and character-level comparisons ----
    uint32_t block_eq(uint32_t a, uint32_t b, bool want_equal);            // bivariate LUT on lhs * M + rhs
    uint32_t packed_pair_eq(uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b);    // two blocks per PBS through the padding bit
    bool packed_pair_fits(uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b) const;
    // equality bits of two encrypted chars: bpc bits (reference shape) or bpc/2 bits (packed)
    std::vector<uint32_t> char_eq_bits(const std::vector<uint32_t>& x, const std::vector<uint32_t>& y);
    // 0/1 blocks saying char == clear byte (want_equal) / != per packed pair
    std::vector<uint32_t> char_scalar_bits(const std::vector<uint32_t>& blocks, uint8_t v, bool want_equal);
    uint32_t char_is_zero(const std::vector<uint32_t>& blocks);            // compare_blocks_with_zero: one 0/1 block, char == 0
    std::vector<Term> nibble_terms(const std::vector<uint32_t>& b, bool high) const;    // one nibble as a lookup input: half of the blocks
    // two-level classify: hi_lut on the high nibble, lo_lut on the low one, comb on 4 * hi + lo
    uint32_t classify_nibbles(const std::vector<uint32_t>& b, uint32_t hi_lut, uint32_t lo_lut, uint32_t comb);

    // ---- gates and selects ----
    uint32_t not_bit(uint32_t bit) { return c.lin({{bit, -1}}, 1, 1); }
    std::vector<uint32_t> not_bits(std::vector<uint32_t> bits) { for (uint32_t& b : bits) b = not_bit(b); return bits; }
    uint32_t and_bits(uint32_t a, uint32_t b);                             // one lookup, x == 2; a bit known at build time drops out
    uint32_t and_all(const std::vector<uint32_t>& bits);                   // AND in one lookup (sum against number); known bits drop out
    uint32_t gate_block(uint32_t block, uint32_t bit, bool keep_if_set);   // block * bit (or * NOT bit): LUT on bit + 2 * block
    uint32_t scale_bit(uint32_t bit, uint32_t v);                          // bit * (clear block v): one lookup on the bit
    // sel ? b : a for two blocks in [0, hi] in ONE lookup where it fits (the result keeps a's noise plus one variance)
    uint32_t select_block(uint32_t a, uint32_t b, uint32_t sel, uint32_t hi);
    // sel ? a : b as two gates and their sum (if_then_else without the final message_extract, integer/.../cmux.rs:194-248)
    uint32_t select_gated(uint32_t sel, uint32_t a, uint32_t b) { return c.lin({{gate_block(a, sel, true), 1}, {gate_block(b, sel, false), 1}}, 0, M - 1); }

    // ---- combining results ("Combining results") ----
    // AND / OR / XOR of any number of bits: bits known at build time drop out; what is left is summed in groups one lookup
    // holds (two bits: one lookup); a linear bit -- a NOT -- enters the sums as it is
    uint32_t combine_bits(const std::vector<uint32_t>& bits, opname::How how);
    // sel ? a : b, each side cut or zero-padded to `cap` characters (fit): one lookup per block where select_block fits
    Str select(uint32_t sel, const Str& a, const Str& b, uint32_t cap);
    // the same on two digit vectors (little endian, the shorter one extended with zeros)
    std::vector<uint32_t> select_digits(uint32_t sel, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b);
    // every output block of a stand-alone combining plan is a lookup's result (as settle): one that no lookup has gone into
    // -- an input, its negation -- goes through the identity, one known at build time becomes a constant table read on
    // `anchor`, an input of the plan
    void settle_combined(std::vector<uint32_t>& blocks, uint32_t anchor);

    // ---- shapes: case, whitespace, trims, shifts, concatenation, length ----
    Str change_case(const Str& s, bool to_lower);
    std::vector<uint32_t> whitespace_bits(const Str& s, bool null_too);    // [s[i] is ASCII whitespace] (+ [s[i] == 0])
    Str trim_end(const Str& s);
    Str trim_start(const Str& s);
    // shift left by the number of leading ones of the monotone indicator `lead` (barrel shifter)
    Str shift_left_by_leading(const Str& s, std::vector<uint32_t> lead);
    // a ++ b without a's padding, capacity a.cap + b.cap.  with_occ: both are left-justified with per-slot occupancy bits
    // (.occ), which replace the char_is_zero tests and travel as one more block
    Str concat(const Str& a, const Str& b, bool with_occ = false);
    Str concat_tree(std::vector<Str> pieces) {                             // left-justified pieces with occupancy bits, pairwise
        return tree_reduce(std::move(pieces), [&](const Str& a, const Str& b) { return concat(a, b, true); })[0];
    }
    uint32_t is_empty(const Str& s) { return char_is_zero(s.ch[0]); }
    std::vector<uint32_t> len(const Str& s, uint32_t n_digits);            // base-M digits of the offset of the first null char

    // ---- equality and order (str_match.cpp) ----
    uint32_t eq(const Str& a, const Operand& b, bool want_equal);
    uint32_t compare_sign(const Str& a, const Operand& b);                 // 0 = a < b, 1 = equal, 2 = a > b
    uint32_t order_bit(uint32_t sign, const std::string& op);              // lt / le / gt / ge read off the sign
    // ---- pattern matching (str_match.cpp) ----
    // encrypted, zero padded pattern: match[o] for o in [0, n_off) = AND_i [s[o+i] matches pat[i]]; padding_wildcard: the
    // pattern's padding matches anything; need_end: the string must end right after the window
    std::vector<uint32_t> window_matches(const Str& s, const Str& pat, uint32_t n_off, bool padding_wildcard, bool need_end = false);
    GroupWeights group_weights(uint32_t k, uint32_t n) const;             // k pattern characters of n equality bits each in one lookup
    uint32_t group_size(uint32_t n, uint32_t remaining) const;            // how many the box and the budget allow
    // clear pattern: match[o] = AND_{i<len} [s[o+i] == pat[i]], o + len <= cap (_classes: whole characters classified;
    // false where that does not fit)
    bool window_matches_clear_classes(const Str& s, const uint8_t* pat, uint32_t len, uint32_t n_off, std::vector<uint32_t>& match);
    std::vector<uint32_t> window_matches_clear(const Str& s, const uint8_t* pat, uint32_t len, uint32_t n_off);
    // cand[o] = match[o] (a window of len characters at o) and the string ends right behind it, 0 < len <= s.cap
    std::vector<uint32_t> ending_here(const Str& s, const std::vector<uint32_t>& match, uint32_t len);
    uint32_t starts_with(const Str& s, const Operand& pat);
    uint32_t contains(const Str& s, const Operand& pat);
    uint32_t ends_with(const Str& s, const Operand& pat);
    // strip_prefix / strip_suffix: the string without the pattern where it has it; *stripped_bit says whether
    Str strip_prefix(const Str& s, const Operand& pat, uint32_t* stripped_bit);
    Str strip_suffix(const Str& s, const Operand& pat, uint32_t* stripped_bit);
    // ---- OR-scans and find (str_match.cpp) ----
    uint32_t scan_run() const { return full_box_reduce ? T : T - 1; }      // bits per run of a scan (T: Circuit::pbs_full_box)
    // the scan inside runs of scan_run() bits: within[j] = OR of j's run up to j, tot[b] = OR of run b
    struct RunScan { std::vector<uint32_t> within, tot; };
    RunScan scan_runs(const std::vector<uint32_t>& bits);
    std::vector<uint32_t> prefix_or(const std::vector<uint32_t>& bits);        // out[o] = OR_{o' <= o} bits[o']
    std::vector<uint32_t> prefix_or_known(const std::vector<uint32_t>& bits);  // the same, known zeros at both ends kept out
    // found bit, then n_digits base-M digits (little endian) of the first (from_end: last) matching offset
    std::vector<uint32_t> find_from_matches(const std::vector<uint32_t>& match, uint32_t n_digits, bool from_end = false);

    // ---- occurrences and replace (str_replace.cpp) ----
    bool occurrences_scan(const std::vector<uint32_t>& match, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf, Occurrences& oc);
    // leftmost non-overlapping occurrences of a pattern of length m among match[]; nzf: see Occurrences
    Occurrences occurrences(const std::vector<uint32_t>& match, uint32_t m, uint32_t n_chars, bool may_overlap, const std::vector<uint32_t>* nzf);
    // cover[i] = [character i lies inside a selected occurrence], forward from the selection whatever produced it
    std::vector<uint32_t> cover_from_sel(const std::vector<uint32_t>& sel, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf);
    // equal lengths (|from| = |to| = m, `to` clear or unpadded encrypted): every covered character rewritten in place
    Str replace_in_place(const Str& s, const Occurrences& oc, uint32_t m, const Operand& to);
    // any lengths: pieces per position, concatenated pairwise, cut / padded to out_cap
    Str replace_general(const Str& s, const Occurrences& oc, const Operand& to, uint32_t out_cap);
    Str replace_empty_pattern(const Str& s, const uint8_t* to_clear, uint32_t t, uint32_t out_cap);    // `to` around every character
    static bool has_border(const uint8_t* p, uint32_t m);                  // proper prefix == suffix => matches may overlap
    // replacen: only the first n selected occurrences stay selected (counted: n encrypted, thermometer g); cover follows
    void keep_first_occurrences(Occurrences& oc, uint32_t n, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf);
    void keep_counted_occurrences(Occurrences& oc, const std::vector<uint32_t>& g, uint32_t m, uint32_t n_chars, const std::vector<uint32_t>* nzf);

    // ---- split family and encrypted counts (str_split.cpp) ----
    // ge[q - 1][i] = [at least q of marks[0..i] are set], q = 1..Q
    std::vector<std::vector<uint32_t>> count_ge(const std::vector<uint32_t>& marks, uint32_t Q);
    // the characters of s where in[i] is set (contiguous or absent), moved to the front, part_cap characters
    Str extract_part(const Str& s, const std::vector<uint32_t>& in, uint32_t part_cap);
    void emit_count(const std::vector<uint32_t>& unary, uint32_t max_value);   // outputs the digits of sum(unary), unary monotone
    std::vector<uint32_t> count_inputs(uint32_t n_max);                    // the digits of an encrypted count with public bound n_max, as inputs
    // g[q - from] = [n >= q], q = from .. n_max (from = 1: the whole thermometer)
    std::vector<uint32_t> count_thermometer(const std::vector<uint32_t>& digits, uint32_t n_max, uint32_t from = 1);
    // selected occurrences of the pattern in s, leftmost or rightmost first, and the characters they cover; sel has s.cap entries
    Occurrences select_occurrences(const Str& s, const Operand& pat, bool from_right);
    // outputs: the count digits (split_once / rsplit_once: the found bit), then P parts of part_cap characters
    // g (splitn_encn / rsplitn_encn only): the thermometer of the encrypted n, P entries
    void split(const Str& s, const SplitKind& kind, const Operand& pat, uint32_t P, uint32_t part_cap, const std::vector<uint32_t>* g = nullptr);

    // ---- slicing at a position: take, skip, char_at, insert (str_slice.cpp) ----
    // the bits of min(n, bound), least significant first: as many as `bound` has; bound < M^D for D digits
    std::vector<uint32_t> count_bits(const std::vector<uint32_t>& digits, uint32_t bound);
    Str take(const Str& s, const Position& at, uint32_t cap);             // s[:n]: min(cap, s.cap, n) characters
    Str skip(const Str& s, const Position& at);                           // s[n:], left-justified
    std::vector<uint32_t> char_at(const Str& s, const Position& at);      // the bit [n < len(s)], then the blocks of s[n:n+1]
    Str insert(const Str& s, const Position& at, const Operand& t, uint32_t cap);    // s[:n] + t + s[n:], cut or padded to cap
    // every output block of a slice is a lookup's result: a bare input goes through the identity
    void settle(std::vector<uint32_t>& blocks);

    // ---- matches: a clear regular expression (str_regex_match.cpp) ----
    uint32_t gated_or(std::vector<uint32_t> bits, uint32_t gate);          // gate AND (OR of bits), in one lookup where that fits
    bool matches_fits() const;                                             // can the per-character class lookups be built?
    uint32_t matches(const Str& a, const regex::Automaton& g);
};

// The cover computation of one selection: which selected occurrence still runs at which character (str_replace.cpp).
struct RunCover {
    StrOps& ops;
    const std::vector<uint32_t>& sel;
    const std::vector<uint32_t>* nzf;
    RunMemo running;
    uint32_t running_bit(uint32_t o, uint32_t j);                          // sel[o] AND nzf[j], memoised
    std::vector<uint32_t> cover(uint32_t m, uint32_t n_chars);
};

inline void append(std::vector<uint32_t>& to, const std::vector<uint32_t>& from) { to.insert(to.end(), from.begin(), from.end()); }

}  // namespace fhe
