// str_op_name.h -- the names of the FheString plans: the one parser and the one table.
//
// A plan name is  base[_reference][_clear][:p1[:p2[:p3]]]  ("eq", "find_reference_clear", "replacen_encn_clear:2:1:8",
// "split_once:3", "skip_encn:32", "matches_clear").  build_string_op (fhe_string.cpp), the layout table of string programs
// (str_program.cpp) and the C ABI's split entry points (c_api.cpp) all read names through parse() and find_row(); nothing else
// compares a name.  Standard headers only (tests/test_program_host.py compiles this stand-alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace fhe {
namespace opname {

enum Family : uint8_t { COMPARE, ORDER, AFFIX, FIND, STRIP_BIT, UNARY_STRING, LEN, IS_EMPTY, CONCAT, REPEAT, REPLACE, SPLIT, MATCHES, SLICE };
enum Form : uint8_t { ENC = 1, CLR = 2, UNARY = 4 };         // an encrypted second operand / a clear one (name_clear) / none
// Which member of its family a row is, where the family has several (the order family passes its name to order_bit):
// eq / ne / eq_ignore_case, where an affix, a search, a strip or a trim works, the case, replace / replacen / replacen_encn,
// the operation of the slice family.
enum How : uint8_t { AS_NAMED, NEGATED, IGNORE_CASE, AT_START, AT_END, ANYWHERE, UPPER, LOWER, BOTH_ENDS, FIRST_N, COUNTED,
                     TAKE, SKIP, SPLIT_AT, CHAR_AT, INSERT };
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
    // repeat:<n_max>: the encrypted-count form of repeat_clear; its inputs are the string and the count's digits
    bool counted_repeat() const { return is(REPEAT) && !clear && !params.empty(); }
};
// A parameter is 1 to 9 decimal digits.  _reference, _reference_clear and _clear are suffixes only of a longer name.
Name parse(const std::string& op);

uint32_t blocks_per_char(uint32_t msg_mod);                  // 8 / b for msg_mod = 2^b with b | 8, else 0
uint32_t count_digits(uint32_t msg_mod, uint64_t n_max);     // the smallest D with msg_mod^D > n_max

}  // namespace opname
}  // namespace fhe
