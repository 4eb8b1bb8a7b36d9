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
    // the families that combine results; a condition bit is the last input.  Every row takes a parameter: none is bare.
    Row("and", LOGIC, UNARY, 1, false, L_AND),                          // name:k: k bits (k >= 2) -> one bit
    Row("or", LOGIC, UNARY, 1, false, L_OR),
    Row("xor", LOGIC, UNARY, 1, false, L_XOR),
    Row("not", LOGIC, UNARY, 1, false, L_NOT),                          // not:k: k bits (k >= 1) -> k bits
    Row("select", SELECT, ENC | CLR, 1, false, OF_STRINGS),             // select[_clear]:C: a, b (or clear bytes), bit -> string
    Row("select_count", SELECT, ENC, 2, false, OF_COUNTS),              // select_count:a_max:b_max: digits, digits, bit -> count
    Row("count_add", COUNT, ENC | CLR, 2, false, C_ADD),                // name:a_max:b_max, name_clear:a_max (the integer: 1..4 clear bytes)
    Row("count_sub", COUNT, ENC | CLR, 2, false, C_SUB),
    Row("count_eq", COUNT, ENC | CLR, 2, false, C_EQ),
    Row("count_ne", COUNT, ENC | CLR, 2, false, C_NE),
    Row("count_lt", COUNT, ENC | CLR, 2, false, C_LT),
    Row("count_le", COUNT, ENC | CLR, 2, false, C_LE),
    Row("count_gt", COUNT, ENC | CLR, 2, false, C_GT),
    Row("count_ge", COUNT, ENC | CLR, 2, false, C_GE),
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

int combine_shape(const Name& n, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, Combine& out, std::string& why) {
    out = Combine();
    const Row& row = *n.row;
    const std::string base = row.name, op = base + (n.clear ? "_clear" : "");
    auto refuse = [&](const std::string& reason) { why = reason; return 1; };
    if (n.clear && !(row.forms & CLR)) return refuse(op + ": " + base + " has no _clear form (select and the count_ names have one)");
    if (row.family != SELECT || row.how == OF_COUNTS) {
        if (a_cap || b_cap) return refuse(op + " takes no string: a_cap and b_cap must be 0");
    } else {
        if (a_cap == 0) return refuse(op + ": the string capacity must be > 0");
        if (!n.clear && b_cap == 0) return refuse("select: the second string needs a capacity of at least one character (clear bytes: select_clear)");
        if (n.clear && b_cap) return refuse("select_clear takes one encrypted string, the other is the clear bytes: b_cap must be 0");
    }
    const std::vector<uint32_t>& p = n.params;
    switch (row.family) {
    case LOGIC: {
        if (p.size() != 1) return refuse(op + " takes one parameter: the number of bits k");
        const uint32_t least = row.how == L_NOT ? 1 : 2;
        if (p[0] < least) return refuse(op + ": k must be at least " + std::to_string(least));
        if (p[0] > (1u << 16)) return refuse(op + ": k must be at most 65536");
        out.operands.assign(p[0], Piece{A_BIT, 1});
        out.results.assign(row.how == L_NOT ? p[0] : 1, Piece{A_BIT, 1});
        return 0;
    }
    case SELECT:
        if (row.how == OF_COUNTS) {
            if (p.size() != 2) return refuse(op + " takes two parameters: the bounds a_max and b_max");
            if (p[0] == 0 || p[1] == 0) return refuse(op + ": a bound must be at least 1");
            out.operands = {Piece{A_COUNT, p[0]}, Piece{A_COUNT, p[1]}, Piece{A_BIT, 1}};
            out.results = {Piece{A_COUNT, p[0] > p[1] ? p[0] : p[1]}};
            return 0;
        }
        if (p.size() != 1) return refuse(op + " takes one parameter: the output capacity C");
        if (p[0] == 0) return refuse(op + ": the output capacity must be > 0");
        out.operands.push_back(Piece{A_STRING, a_cap});
        if (!n.clear) out.operands.push_back(Piece{A_STRING, b_cap});
        out.operands.push_back(Piece{A_BIT, 1});
        out.results = {Piece{A_STRING, p[0]}};
        return 0;
    case COUNT: {
        if (p.size() != (n.clear ? 1u : 2u))
            return refuse(n.clear ? op + " takes one parameter: the bound a_max (the second operand is the clear integer)"
                                  : op + " takes two parameters: the bounds a_max and b_max");
        if (p[0] == 0 || (!n.clear && p[1] == 0)) return refuse(op + ": a bound must be at least 1");
        uint64_t scalar = 0;
        if (n.clear) {
            if (clear_len < 1 || clear_len > 4 || !clear)
                return refuse(op + ": the clear integer is 1 to 4 little-endian bytes, got " + std::to_string(clear_len));
            for (uint32_t i = 0; i < clear_len; i++) scalar |= (uint64_t)clear[i] << (8 * i);
        }
        out.scalar = (uint32_t)scalar;
        out.operands.push_back(Piece{A_COUNT, p[0]});
        if (!n.clear) out.operands.push_back(Piece{A_COUNT, p[1]});
        const uint64_t sum = (uint64_t)p[0] + (n.clear ? scalar : p[1]);
        if (row.how == C_ADD && sum > 0xFFFFFFFFull) return refuse(op + ": the bound of the sum must stay below 2^32");
        out.results = {row.how == C_ADD ? Piece{A_COUNT, (uint32_t)sum} : row.how == C_SUB ? Piece{A_COUNT, p[0]} : Piece{A_BIT, 1}};
        return 0;
    }
    default: return refuse("internal: " + op + " is no combining name");
    }
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
