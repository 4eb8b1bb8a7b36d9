// str_op_name.h -- the names of the FheString plans: the one parser and the one table.
//
// A plan name is  base[_reference][_clear][:p1[:p2[:p3]]]  ("eq", "find_reference_clear", "replacen_encn_clear:2:1:8",
// "split_once:3", "skip_encn:32", "matches_clear", "and:2", "select:8", "count_add_clear:8").  build_string_op (fhe_string.cpp), the layout table of string programs
// (str_program.cpp) and the C ABI's split entry points (c_api.cpp) all read names through parse() and find_row(); nothing else
// compares a name.  Standard headers only (tests/test_program_host.py compiles this stand-alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace fhe {
namespace opname {

enum Family : uint8_t { COMPARE, ORDER, AFFIX, FIND, STRIP_BIT, UNARY_STRING, LEN, IS_EMPTY, CONCAT, REPEAT, REPLACE, SPLIT, MATCHES, SLICE,
                       LOGIC, SELECT, COUNT };
enum Form : uint8_t { ENC = 1, CLR = 2, UNARY = 4 };         // an encrypted second operand / a clear one (name_clear) / none
// Which member of its family a row is, where the family has several (the order family passes its name to order_bit):
// eq / ne / eq_ignore_case, where an affix, a search, a strip or a trim works, the case, replace / replacen / replacen_encn,
// the operation of the slice family and of the families that combine results.
enum How : uint8_t { AS_NAMED, NEGATED, IGNORE_CASE, AT_START, AT_END, ANYWHERE, UPPER, LOWER, BOTH_ENDS, FIRST_N, COUNTED,
                     TAKE, SKIP, SPLIT_AT, CHAR_AT, INSERT,
                     // the bit logic, what a select chooses between, the arithmetic and the comparisons of two counts
                     L_AND, L_OR, L_XOR, L_NOT, OF_STRINGS, OF_COUNTS, C_ADD, C_SUB, C_EQ, C_NE, C_LT, C_LE, C_GT, C_GE };
enum Split : uint8_t { REVERSE = 1, TERMINATOR = 2, INCLUSIVE = 4, LIMITED = 8, ONCE = 16, WHITESPACE = 32, ENC_COUNT = 64 };

// Which operation of the split family: see include/fhestr.h for the semantics of each.
struct SplitKind {
    bool reverse, terminator, inclusive, limited, once, whitespace;
    bool enc_count;                // splitn_encn / rsplitn_encn: n is encrypted, max_parts is its public bound; the _encn
                                   // rows of the slice family: the position is encrypted, the first parameter its bound
    constexpr SplitKind(unsigned f = 0) : reverse(f & REVERSE), terminator(f & TERMINATOR), inclusive(f & INCLUSIVE), limited(f & LIMITED),
                                          once(f & ONCE), whitespace(f & WHITESPACE), enc_count(f & ENC_COUNT) {}
};

struct Row {
    const char* name;
    Family family;
    uint8_t forms;                 // Form bits
    // The name takes `params` numeric parameters; bare: it also builds without any.  The last parameter of a split
    // row, the part capacity, and the output capacity of a slice row with two parameters may be left out.  Rows with
    // params = 0 ignore parameters (matches_clear refuses them).
    uint8_t params;
    bool bare;
    How how;
    SplitKind split;               // SPLIT rows
    constexpr Row(const char* name, Family family, unsigned forms, unsigned params, bool bare, How how = AS_NAMED, unsigned split = 0)
        : name(name), family(family), forms((uint8_t)forms), params((uint8_t)params), bare(bare), how(how), split(split) {}
    bool unary() const { return forms & UNARY; }
    bool takes(size_t n_params) const {
        return n_params == params || (bare && n_params == 0) || (family == SPLIT && n_params + 1 == params) ||
               (family == SLICE && params == 2 && n_params == 1);
    }
};

const Row* find_row(const std::string& base);                // the row of the table (str_op_name.cpp); null: not a base name

enum Status { OK, BAD_PARAMETER, NOT_A_NAME };
struct Name {
    Status status = NOT_A_NAME;
    const Row* row = nullptr;      // the base's row; null unless status == OK
    bool clear = false, reference = false;                   // the suffixes, also of a name whose base has no row
    std::vector<uint32_t> params;
    bool is(Family f) const { return row && row->family == f; }
    // the families that combine results (bit logic, select, count arithmetic): their operands are bits and counts as well
    // as strings, in the order the row's comment gives
    bool combines() const { return is(LOGIC) || is(SELECT) || is(COUNT); }
    // repeat:<n_max>: the encrypted-count form of repeat_clear; its inputs are the string and the count's digits
    bool counted_repeat() const { return is(REPEAT) && !clear && !params.empty(); }
};
// A parameter is 1 to 9 decimal digits.  _reference, _reference_clear and _clear are suffixes only of a longer name.
Name parse(const std::string& op);

// What a name of the combining families takes and returns: strings (extent = the capacity), bits (1) and counts (the public
// bound), the operands in the order of the plan's inputs.  The kinds are numbered as program::Kind.
enum ValueKind : uint8_t { A_STRING = 0, A_BIT = 1, A_COUNT = 2 };
struct Piece {
    ValueKind kind;
    uint32_t extent;
};
struct Combine {
    std::vector<Piece> operands, results;
    uint32_t scalar = 0;           // the clear integer of a count name's _clear form
};
// The shape of `n` (n.combines()) on strings of a_cap and b_cap characters with `clear_len` clear bytes; nonzero: refused,
// the reason in `why` -- a missing parameter, k = 0, C = 0, a bound of 0, a capacity the name does not use, _clear on a
// name without that form, a clear integer that is not 1 to 4 bytes.
int combine_shape(const Name& n, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, Combine& out, std::string& why);

uint32_t blocks_per_char(uint32_t msg_mod);                  // 8 / b for msg_mod = 2^b with b | 8, else 0
uint32_t count_digits(uint32_t msg_mod, uint64_t n_max);     // the smallest D with msg_mod^D > n_max

}  // namespace opname
}  // namespace fhe
