// str_op_name.cpp -- the table of FheString plan names and their parser (see str_op_name.h).  Standard headers only.
#include "str_op_name.h"

namespace fhe {
namespace opname {

// One row per base name.  tests/test_gpu_exact_plan.py reads the rows (name, family, forms, params, bare) from this file:
// keep one Row(...) per line.
static const Row TABLE[] = {
    Row("eq", COMPARE, ENC | CLR, 0, true),
    Row("ne", COMPARE, ENC | CLR, 0, true, NEGATED),
    Row("eq_ignore_case", COMPARE, ENC | CLR, 0, true, IGNORE_CASE),
    Row("lt", ORDER, ENC | CLR, 0, true),
    Row("le", ORDER, ENC | CLR, 0, true),
    Row("gt", ORDER, ENC | CLR, 0, true),
    Row("ge", ORDER, ENC | CLR, 0, true),
    Row("starts_with", AFFIX, ENC | CLR, 0, true, AT_START),
    Row("ends_with", AFFIX, ENC | CLR, 0, true, AT_END),
    Row("contains", AFFIX, ENC | CLR, 0, true, ANYWHERE),
    Row("find", FIND, ENC | CLR, 0, true, AT_START),
    Row("rfind", FIND, ENC | CLR, 0, true, AT_END),
    Row("strip_prefix", STRIP_BIT, ENC | CLR, 0, true, AT_START),
    Row("strip_suffix", STRIP_BIT, ENC | CLR, 0, true, AT_END),
    Row("to_upper", UNARY_STRING, UNARY, 0, true, UPPER),
    Row("to_lower", UNARY_STRING, UNARY, 0, true, LOWER),
    Row("trim_start", UNARY_STRING, UNARY, 0, true, AT_START),
    Row("trim_end", UNARY_STRING, UNARY, 0, true, AT_END),
    Row("strip", UNARY_STRING, UNARY, 0, true, BOTH_ENDS),
    Row("trim", UNARY_STRING, UNARY, 0, true, BOTH_ENDS),               // = strip
    Row("len", LEN, UNARY, 0, true),
    Row("is_empty", IS_EMPTY, UNARY, 0, true),
    Row("concat", CONCAT, ENC | CLR, 0, true),
    Row("repeat", REPEAT, CLR, 1, true),                                // repeat_clear (the count in the clear byte), repeat:<n_max>
    Row("replace", REPLACE, ENC | CLR, 2, true),                        // replace[_clear][:F:C]: default F = half, C = a_cap
    Row("replacen", REPLACE, ENC | CLR, 3, false, FIRST_N),             // replacen[_clear]:n:F:C
    Row("replacen_encn", REPLACE, ENC | CLR, 3, false, COUNTED),        // replacen_encn[_clear]:n_max:F:C
    Row("split", SPLIT, ENC | CLR, 2, false),                           // name[_clear]:P[:C]
    Row("rsplit", SPLIT, ENC | CLR, 2, false, AS_NAMED, REVERSE),
    Row("split_terminator", SPLIT, ENC | CLR, 2, false, AS_NAMED, TERMINATOR),
    Row("rsplit_terminator", SPLIT, ENC | CLR, 2, false, AS_NAMED, REVERSE | TERMINATOR),
    Row("split_inclusive", SPLIT, ENC | CLR, 2, false, AS_NAMED, INCLUSIVE),
    Row("splitn", SPLIT, ENC | CLR, 2, false, AS_NAMED, LIMITED),
    Row("rsplitn", SPLIT, ENC | CLR, 2, false, AS_NAMED, REVERSE | LIMITED),
    Row("splitn_encn", SPLIT, ENC | CLR, 2, false, AS_NAMED, LIMITED | ENC_COUNT),
    Row("rsplitn_encn", SPLIT, ENC | CLR, 2, false, AS_NAMED, REVERSE | LIMITED | ENC_COUNT),
    Row("split_once", SPLIT, ENC | CLR, 1, true, AS_NAMED, ONCE),       // name[_clear][:C]
    Row("rsplit_once", SPLIT, ENC | CLR, 1, true, AS_NAMED, REVERSE | ONCE),
    Row("split_ascii_whitespace", SPLIT, UNARY, 2, false, AS_NAMED, WHITESPACE),
    Row("take", SLICE, UNARY, 2, false, TAKE),                          // name:n[:C], name_encn:n_max[:C]: default C = a_cap
    Row("take_encn", SLICE, UNARY, 2, false, TAKE, ENC_COUNT),
    Row("skip", SLICE, UNARY, 2, false, SKIP),
    Row("skip_encn", SLICE, UNARY, 2, false, SKIP, ENC_COUNT),
    Row("split_at", SLICE, UNARY, 2, false, SPLIT_AT),
    Row("split_at_encn", SLICE, UNARY, 2, false, SPLIT_AT, ENC_COUNT),
    Row("char_at", SLICE, UNARY, 1, false, CHAR_AT),                    // char_at:n, char_at_encn:n_max
    Row("char_at_encn", SLICE, UNARY, 1, false, CHAR_AT, ENC_COUNT),
    Row("insert", SLICE, ENC | CLR, 2, false, INSERT),                  // insert[_clear]:n[:C]: default C = a_cap + the capacity / length of t
    Row("insert_encn", SLICE, ENC | CLR, 2, false, INSERT, ENC_COUNT),
    Row("matches", MATCHES, CLR, 0, true),                              // matches_clear: the pattern text /.../ of regex.h
};

const Row* find_row(const std::string& base) {
    for (const Row& row : TABLE)
        if (base == row.name) return &row;
    return nullptr;
}

// true: `s` ends with `tail` and is longer; the tail is cut off
static bool cut_suffix(std::string& s, const std::string& tail) {
    if (s.size() <= tail.size() || s.compare(s.size() - tail.size(), tail.size(), tail) != 0) return false;
    s.resize(s.size() - tail.size());
    return true;
}

Name parse(const std::string& op) {
    Name n;
    const size_t colon = op.find(':');
    std::string base = op.substr(0, colon);
    for (size_t pos = colon; pos != std::string::npos;) {
        const size_t nxt = op.find(':', pos + 1);
        const std::string tok = op.substr(pos + 1, nxt == std::string::npos ? nxt : nxt - pos - 1);
        if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos || tok.size() > 9) {
            n.status = BAD_PARAMETER;
            return n;
        }
        n.params.push_back((uint32_t)std::stoul(tok));
        pos = nxt;
    }
    // the reference's circuit shape: name_reference, name_reference_clear (and name_clear_reference)
    if (cut_suffix(base, "_reference_clear")) n.reference = n.clear = true;
    else n.reference = cut_suffix(base, "_reference");
    if (!n.clear) n.clear = cut_suffix(base, "_clear");
    n.row = find_row(base);
    if (n.row) n.status = OK;
    return n;
}

uint32_t blocks_per_char(uint32_t msg_mod) {
    uint32_t bits = 0;
    while (bits < 8 && (1u << bits) < msg_mod) bits++;
    return bits && (1u << bits) == msg_mod && 8 % bits == 0 ? 8 / bits : 0;
}

uint32_t count_digits(uint32_t msg_mod, uint64_t n_max) {
    uint32_t d = 1;
    for (uint64_t span = msg_mod; span <= n_max; span *= msg_mod) d++;
    return d;
}

}  // namespace opname
}  // namespace fhe
