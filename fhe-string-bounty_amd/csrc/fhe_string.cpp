// fhe_string.cpp -- FheString operations as batched shortint circuits: the op dispatch behind the C ABI.
//
// The reference snapshot has no FheString type; its building blocks are the integer
// layer's block-wise comparison loops, restated on whole strings by StrOps (str_ops.h and the units it names):
//   unchecked_eq / unchecked_ne            integer/server_key/radix_parallel/comparison.rs:10-83
//   unchecked_scalar_eq / _ne (+ packing)  .../scalar_comparison.rs:104-138,366-558
//   are_all_comparisons_block_true         .../scalar_comparison.rs:147-191
//   is_at_least_one_comparisons_block_true .../scalar_comparison.rs:200-233
//   compare_blocks_with_zero               .../scalar_comparison.rs:254-296
// and the char-wise patterns of the docs tutorial / regex engine
// (tfhe/docs/tutorials/ascii_fhe_string.md:84-131, tfhe/examples/regex_engine/execution.rs:63-86).
#include <string>

#include "count_ops.h"
#include "str_ops.h"

namespace fhe {


// ------------------------------------------------------------------------------------------------
// op dispatch used by the C ABI: builds the circuit for `op` and declares its outputs.  The names and their grammar are
// defined in str_op_name.cpp.  The names that combine results (bit logic, select, count arithmetic) take bits and counts as
// well as strings and are built by build_combined.  For every other name build_string_op parses the name, runs the
// refusals that every family shares, creates the inputs -- a, then b; the digits of an encrypted count come last, from the
// family's own function after its parameter checks -- and OpBuilder::build switches on the family of the name's row.
namespace {
using opname::AT_END;
using opname::AT_START;

struct OpBuilder {
    Circuit& c;
    StrOps& s;
    const opname::Name& n;
    const opname::Row& row;
    const Str &a, &b;                    // b: without characters for a clear, a unary and a counted form
    const uint8_t* clear;
    const uint32_t clear_len, a_cap;
    const Operand rhs;                   // the right operand as the operations take it: b, or the clear bytes
    // an encrypted count: its digits are the plan's last inputs, after the string and the encrypted pattern operand(s)
    std::vector<uint32_t> count_g;
    void take_count(uint32_t n_max) { count_g = s.count_thermometer(s.count_inputs(n_max), n_max); }
    uint32_t n_digits() const { return opname::count_digits(s.M, a_cap); }          // the digits that hold 0 .. a_cap
    void output(const std::vector<uint32_t>& outs) { for (uint32_t o : outs) c.output(o); }

    int build_matches() {         // clear = the pattern text /.../ of the reference's regex engine (regex.h)
        if (!n.params.empty()) return fail("matches_clear takes no parameters");
        regex::Automaton g;
        std::string why;
        if (regex::compile(clear, clear_len, g, why)) return fail("matches_clear: " + why);
        if (g.literal().empty() && !s.matches_fits())
            return fail("matches_clear needs a nibble of a character as one lookup input: msg_mod * carry_mod >= 16 within the noise budget");
        c.output(s.matches(a, g));
        return 0;
    }
    uint32_t compare() {
        if (row.how != opname::IGNORE_CASE) return s.eq(a, rhs, row.how != opname::NEGATED);
        if (!n.clear) return s.eq(s.change_case(a, true), s.change_case(b, true), true);
        std::vector<uint8_t> lower(clear, clear + clear_len);
        for (auto& ch : lower) if (ch >= 'A' && ch <= 'Z') ch += 32;
        return s.eq(s.change_case(a, true), Operand(lower.data(), clear_len), true);
    }
    void build_strip_bit() {
        uint32_t bit = 0;
        const Str r = row.how == AT_START ? s.strip_prefix(a, rhs, &bit) : s.strip_suffix(a, rhs, &bit);
        c.output(bit);          // first output: 1 iff the pattern was stripped
        s.emit(r);
    }
    void build_find() {
        const bool from_end = row.how == AT_END;
        std::vector<uint32_t> match, outs;
        if (n.clear) {
            if (clear_len > a_cap) match.assign(1, c.trivial(0));
            else if (clear_len == 0) match.assign(1, c.trivial(1));
            else match = s.window_matches_clear(a, clear, clear_len, a_cap - clear_len + 1);
        } else {
            match = s.window_matches(a, b, a_cap, true);
            if (from_end) {
                // an (all-padding) pattern also "matches" past the end of the string: only offsets
                // o <= len(s) count, i.e. o == 0 or s[o-1] != 0
                const uint32_t both = s.lut_equals(1);
                for (uint32_t o = 1; o < match.size(); o++)
                    match[o] = c.pbs(c.lin({{match[o], 1}, {s.char_is_zero(a.ch[o - 1]), 2}}, 0, 3), both);
                // ... and an empty pattern matches at offset cap when the string fills its capacity
                // (bytes.rfind(b"") == len): pattern empty AND s[cap-1] != 0
                match.push_back(c.pbs(c.lin({{s.char_is_zero(b.ch[0]), 1}, {s.char_is_zero(a.ch[a_cap - 1]), 2}}, 0, 3), both));
            }
        }
        if (from_end && n.clear && clear_len == 0) {       // "".rfind in s == len(s)
            outs.push_back(c.trivial(1));
            append(outs, s.len(a, n_digits()));
        } else {
            outs = s.find_from_matches(match, n_digits(), from_end);
        }
        output(outs);
    }
    void build_unary_string() {
        switch (row.how) {
        case AT_START: return s.emit(s.trim_start(a));
        case AT_END: return s.emit(s.trim_end(a));
        case opname::BOTH_ENDS: return s.emit(s.trim_start(s.trim_end(a)));
        default: return s.emit(s.change_case(a, row.how == opname::LOWER));
        }
    }
    int build_repeat() {
        if (!n.counted_repeat()) {      // clear repetition count in clear[0] (>= 1): out capacity = count * a_cap
            if (!n.clear || clear_len != 1 || clear[0] == 0) return fail("repeat_clear takes one clear byte: the count (>= 1)");
            Str r = a;
            for (uint32_t i = 1; i < clear[0]; i++) r = s.concat(r, a);
            s.emit(r);
            return 0;
        }
        // copy i is masked by [n >= i + 1] before it is appended: zeroing the tail copies leaves a left-justified result
        if (n.params.size() != 1) return fail("repeat takes one parameter: the count's bound n_max");
        const uint32_t n_max = n.params[0];
        if (n_max == 0 || n_max > 255) return fail("repeat: n_max must be in 1..255");
        take_count(n_max);
        Str r;
        for (uint32_t i = 0; i < n_max; i++) {
            const Str copy = s.build_str(a_cap, [&](uint32_t j, uint32_t k) {
                StrOps::Scope sc(c, s.owner_for(j, a_cap));
                return s.gate_block(a.ch[j][k], count_g[i], true);
            });
            r = i ? s.concat(r, copy) : copy;
        }
        s.emit(r);
        return 0;
    }
    int build_split() {           // P = max_parts (splitn / rsplitn: n; split_once: two parts), C = capacity of every part (default a_cap)
        const opname::SplitKind& kind = row.split;
        if (!row.takes(n.params.size()))
            return fail(kind.once ? "split_once takes at most one parameter: the part capacity"
                                  : "split takes one or two parameters: max_parts and the part capacity");
        const uint32_t P = kind.once ? 2 : n.params[0];
        const uint32_t part_cap = n.params.size() == row.params ? n.params.back() : a_cap;
        if (P == 0) return fail(kind.limited ? "splitn: n must be at least 1" : "split: max_parts must be at least 1");
        if (part_cap == 0) return fail("split: the part capacity must be > 0");
        if (n.clear && clear_len == 0)
            return fail("split: a clear pattern must not be empty (the per-character split of an empty pattern is not supported)");
        if (s.T < 16) return fail("split needs a message * carry space of at least 16 values");
        if (kind.enc_count) take_count(P);
        s.split(a, kind, rhs, P, part_cap, kind.enc_count ? &count_g : nullptr);
        return 0;
    }
    // clear = from (F bytes; default: half) || to, or b = encrypted from (capacity F; default: half) || to; output capacity C
    //   without parameters: equal lengths, encrypted operands fill their capacity, rewritten in place;
    //   with parameters: any lengths, encrypted operands may be zero padded (hidden lengths)
    // replacen, replacen_encn = the general form cut after the first n occurrences (their three parameters are checked already)
    int build_replace() {
        const bool is_replacen = row.how != opname::AS_NAMED, is_replacen_encn = row.how == opname::COUNTED;
        const uint32_t replacen_n = is_replacen ? n.params[0] : 0;
        const std::vector<uint32_t> op_params(n.params.begin() + (is_replacen ? 1 : 0), n.params.end());
        if (!op_params.empty() && op_params.size() != 2) return fail("replace takes two parameters: pattern capacity and output capacity");
        const bool general = !op_params.empty();
        const uint32_t out_cap = general ? op_params[1] : a_cap;
        if (out_cap == 0) return fail("output capacity must be > 0");
        if (is_replacen_encn) take_count(replacen_n);
        auto keep_first_n = [&](Occurrences& oc, uint32_t m, const std::vector<uint32_t>* nzf) {
            if (is_replacen_encn) s.keep_counted_occurrences(oc, count_g, m, a_cap, nzf);
            else if (is_replacen) s.keep_first_occurrences(oc, replacen_n, m, a_cap, nzf);
        };
        if (n.clear) {
            if (!general && clear_len % 2) return fail("replace_clear expects `from` and `to` of equal length, concatenated");
            const uint32_t m = general ? op_params[0] : clear_len / 2;
            if (m > clear_len) return fail("replace_clear: pattern length beyond the clear buffer");
            const uint32_t t = clear_len - m;
            const uint8_t* to = clear + m;
            if (m == 0 && is_replacen) return fail("replacen: a clear pattern must not be empty");
            if (m == 0) s.emit(general ? s.replace_empty_pattern(a, to, t, out_cap) : a);
            else if (m > a_cap || (is_replacen && replacen_n == 0)) s.emit(s.fit(a, out_cap));      // (replacen_encn: n_max >= 1)
            else {
                std::vector<uint32_t> match = s.window_matches_clear(a, clear, m, a_cap - m + 1);
                Occurrences oc = s.occurrences(match, m, a_cap, StrOps::has_border(clear, m), nullptr);
                keep_first_n(oc, m, nullptr);
                s.emit(m == t && out_cap == a_cap ? s.replace_in_place(a, oc, m, Operand(to, t))
                                                  : s.replace_general(a, oc, Operand(to, t), out_cap));
            }
            return 0;
        }
        if (!general && b.cap % 2) return fail("replace expects `from` and `to` of equal capacity, concatenated");
        const uint32_t m = general ? op_params[0] : b.cap / 2;
        if (m == 0 || m > b.cap) return fail("replace: pattern capacity must be in 1..b_cap");
        Str from, to;
        from.cap = m;
        to.cap = b.cap - m;
        from.ch.assign(b.ch.begin(), b.ch.begin() + m);
        to.ch.assign(b.ch.begin() + m, b.ch.end());
        if (!general && m > a_cap) s.emit(a);
        else if (!general) {
            std::vector<uint32_t> match = s.window_matches(a, from, a_cap - m + 1, false);
            Occurrences oc = s.occurrences(match, m, a_cap, true, nullptr);
            s.emit(s.replace_in_place(a, oc, m, to));
        } else if (is_replacen && replacen_n == 0) {
            s.emit(s.fit(a, out_cap));
        } else {
            // padded pattern: its zero tail matches anything; an occurrence runs over from[j] != 0 only.
            // A pattern that decrypts to the empty string selects nothing (nzf[0] = 0).
            std::vector<uint32_t> nzf;
            for (uint32_t j = 0; j < m; j++) nzf.push_back(s.not_bit(s.char_is_zero(from.ch[j])));
            std::vector<uint32_t> match = s.window_matches(a, from, a_cap, true);
            for (uint32_t o = 0; o < match.size(); o++) {
                StrOps::Scope sc(c, s.owner_for(o, (uint32_t)match.size()));
                match[o] = s.and_bits(match[o], nzf[0]);
            }
            Occurrences oc = s.occurrences(match, m, a_cap, true, &nzf);
            keep_first_n(oc, m, &nzf);
            s.emit(s.replace_general(a, oc, to, out_cap));
        }
        return 0;
    }
    // take / skip / split_at / char_at / insert at a clear position n, or (_encn) at an encrypted one with the bound n_max:
    // the first parameter; the second, where the row has one, is the output capacity C (str_slice.cpp)
    int build_slice() {
        const bool enc = row.split.enc_count, inserts = row.how == opname::INSERT;
        const std::string op = row.name, position = enc ? "the position's bound n_max" : "the position n";
        if (n.clear && !inserts) return fail(op + ": _clear is a form of insert only (the clear string to insert)");
        if (!row.takes(n.params.size()))
            return fail(row.params == 1 ? op + " takes one parameter: " + position + " (one character comes back: there is no output capacity)"
                                        : op + " takes one or two parameters: " + position + " and the output capacity");
        if (enc && n.params[0] == 0) return fail(op + ": n_max must be at least 1");
        const uint32_t out_cap = n.params.size() == 2 ? n.params[1] : a_cap + (inserts ? rhs.cap() : 0);
        if (out_cap == 0) return fail(op + ": the output capacity must be > 0");
        if (enc && s.T < 16) return fail(op + " needs a message * carry space of at least 16 values");
        std::vector<uint32_t> digits;
        if (enc) digits = s.count_inputs(n.params[0]);
        const Position at{n.params[0], enc ? &digits : nullptr};
        std::vector<uint32_t> outs;
        auto string = [&](const Str& r) { for (auto& blocks : s.fit(r, out_cap).ch) append(outs, blocks); };
        switch (row.how) {
        case opname::TAKE: string(s.take(a, at, out_cap)); break;
        case opname::SKIP: string(s.skip(a, at)); break;
        case opname::SPLIT_AT: string(s.take(a, at, out_cap)); string(s.skip(a, at)); break;
        case opname::CHAR_AT: outs = s.char_at(a, at); break;
        default: string(s.insert(a, at, rhs, out_cap)); break;
        }
        s.settle(outs);
        // a result known at build time (take:0, a position beyond the capacity) still runs as a plan: one lookup level,
        // a constant table read on the first block of the string
        int64_t known = 0;
        if (c.n_pbs() == 0 && s.is_trivial(outs[0], &known))
            outs[0] = c.pbs(a.ch[0][0], c.lut_fn([known](uint64_t) { return (uint64_t)known; }));
        output(outs);
        return 0;
    }

    int build() {
        switch (row.family) {
        case opname::COMPARE: c.output(compare()); break;
        case opname::ORDER: c.output(s.order_bit(s.compare_sign(a, rhs), row.name)); break;
        case opname::AFFIX: c.output(row.how == AT_START ? s.starts_with(a, rhs) : row.how == AT_END ? s.ends_with(a, rhs) : s.contains(a, rhs)); break;
        case opname::FIND: build_find(); break;
        case opname::STRIP_BIT: build_strip_bit(); break;
        case opname::UNARY_STRING: build_unary_string(); break;
        case opname::LEN: output(s.len(a, n_digits())); break;
        case opname::IS_EMPTY: c.output(s.is_empty(a)); break;
        case opname::CONCAT:         // out capacity = a_cap + (b_cap | clear_len); clear right operand: "concat_clear"
            if (n.clear && clear_len == 0) s.emit(a);
            else s.emit(s.concat(a, n.clear ? s.clear_string(clear, clear_len) : b));
            break;
        case opname::REPEAT: return build_repeat();
        case opname::REPLACE: return build_replace();
        case opname::SPLIT: return build_split();
        case opname::MATCHES: return build_matches();
        case opname::SLICE: return build_slice();
        case opname::LOGIC: case opname::SELECT: case opname::COUNT: break;     // build_combined
        }
        return 0;
    }
};

// The names that combine results ("Combining results").  Inputs in the order of opname::combine_shape;
// a bit is read through linear combinations only, so inside a program a negated bit is bound as it is.  A stand-alone
// plan's outputs are settled; inside a program they stay as built: `not` is linear there and adds no lookup.
int build_combined(Circuit& c, StrOps& s, const opname::Name& n, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len) {
    const opname::Row& row = *n.row;
    opname::Combine shape;
    std::string why;
    if (opname::combine_shape(n, a_cap, b_cap, clear, clear_len, shape, why)) return fail(why);
    const std::string op = std::string(row.name) + (n.clear ? "_clear" : "");
    if (row.family == opname::COUNT && s.T < 16)
        return fail(op + " needs a message * carry space of at least 16 values: the digit sums of a count do not fit a smaller one");
    const bool in_program = c.binding();
    std::vector<Str> strings;
    std::vector<std::vector<uint32_t>> counts;
    std::vector<uint32_t> bits;
    uint32_t anchor = UINT32_MAX;
    for (const opname::Piece& p : shape.operands) {
        if (p.kind == opname::A_STRING) strings.push_back(s.input_string(p.extent));
        else if (p.kind == opname::A_COUNT) counts.push_back(s.count_inputs(p.extent));
        else bits.push_back(c.input_linear(1));
        if (anchor == UINT32_MAX) anchor = p.kind == opname::A_STRING ? strings[0].ch[0][0] : p.kind == opname::A_COUNT ? counts[0][0] : bits[0];
    }
    std::vector<uint32_t> outs;
    switch (row.family) {
    case opname::LOGIC:
        if (row.how == opname::L_NOT) outs = s.not_bits(bits);
        else outs.push_back(s.combine_bits(bits, row.how));
        break;
    case opname::SELECT:
        if (row.how == opname::OF_COUNTS) {
            outs = s.select_digits(bits[0], counts[0], counts[1]);
            break;
        }
        for (auto& blocks : s.select(bits[0], strings[0], n.clear ? s.clear_string(clear, clear_len) : strings[1], n.params[0]).ch) append(outs, blocks);
        break;
    default: {
        const opname::Piece& res = shape.results[0];
        const uint32_t n_out = res.kind == opname::A_BIT ? 1 : opname::count_digits(s.M, res.extent);
        outs = CountOps(c, s).build(row.how, counts[0], n.params[0], n.clear ? nullptr : &counts[1], n.clear ? 0 : n.params[1], shape.scalar, n_out);
        break;
    }
    }
    if (c.failed()) return fail("circuit build error: " + c.error());
    if (!in_program) s.settle_combined(outs, anchor);
    for (uint32_t o : outs) c.output(o);
    return 0;
}
}  // namespace

int build_string_op(Circuit& c, const std::string& op, uint32_t a_cap, uint32_t b_cap,
                    const uint8_t* clear, uint32_t clear_len) {
    StrOps s(c);
    const opname::Name n = opname::parse(op);
    if (n.status == opname::BAD_PARAMETER) return fail("bad numeric parameter in string op: " + op);
    // matches_clear has no encrypted form and no reference-shaped one
    if (n.is(opname::MATCHES) && !n.clear && !n.reference) return fail("matches takes a clear pattern: matches_clear");
    if (n.is(opname::MATCHES) && n.reference) return fail("unknown string op: " + op);
    if (n.reference) {
        s.packed_compare = false;          // the reference's block-by-block circuit shape
        s.full_box_reduce = false;         // ... and its chunks of T - 1 comparison bits
    }
    if (!s.ok) return fail("string ops need msg_mod = 2^b with b | 8 and carry_mod >= msg_mod");
    if (n.combines()) {
        if (n.reference) return fail("unknown string op: " + op);
        if (n.clear && !clear && clear_len) return fail("null clear pattern");
        if (build_combined(c, s, n, a_cap, b_cap, clear, clear_len)) return 1;
        if (c.failed()) return fail("circuit build error: " + c.error());
        return 0;
    }
    if (a_cap == 0) return fail("string capacity must be > 0");
    if (n.clear && !clear && clear_len) return fail("null clear pattern");
    Str a = s.input_string(a_cap);
    Str b;
    if (n.is(opname::SPLIT) && n.row->split.whitespace && (n.clear || clear_len)) return fail("split_ascii_whitespace takes no pattern");
    if (n.is(opname::REPLACE) && n.row->how != opname::AS_NAMED) {
        const bool counted = n.row->how == opname::COUNTED;
        if (!n.row->takes(n.params.size()))
            return fail(counted ? "replacen_encn takes three parameters: the count's bound n_max, the pattern capacity and the output capacity"
                                : "replacen takes three parameters: the count, the pattern capacity and the output capacity");
        if (counted && n.params[0] == 0) return fail("replacen_encn: n_max must be at least 1");
    }
    // repeat:<n_max> takes no b (a bare `repeat` does: it is refused by its family, with the repeat_clear message)
    if (n.counted_repeat() && b_cap) return fail("repeat takes no second string: its inputs are the string and the count's digits");
    if (!n.clear && !(n.row && n.row->unary()) && !n.counted_repeat()) {
        if (b_cap == 0) return fail("pattern capacity must be > 0");
        b = s.input_string(b_cap);
    }
    if (!n.row) return fail("unknown string op: " + op);
    OpBuilder builder{c, s, n, *n.row, a, b, clear, clear_len, a_cap, n.clear ? Operand(clear, clear_len) : Operand(b), {}};
    if (builder.build()) return 1;
    if (c.failed()) return fail("circuit build error: " + c.error());
    return 0;
}

}  // namespace fhe
