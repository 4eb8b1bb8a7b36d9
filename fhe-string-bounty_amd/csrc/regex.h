// regex.h -- clear regular expressions compiled to their position (Glushkov) automaton.
//
// The pattern text is that of the reference's regex engine (tfhe/examples/regex_engine/parser.rs):
//   pattern = '/' '^'? regex '$'? '/' 'i'?          the anchors exist only here and bind looser than '|'
//   regex   = term ('|' regex)?
//   term    = factor+
//   factor  = atom ('?' | '*' | '+' | '{n}' | '{n,}' | '{,m}' | '{n,m}')?
//   atom    = '.' | '\' byte | alphanumeric | one of & ; : , ` ~ - _ ! @ # % ' " | '(' regex ')' | '[' class ']'
//   class   = '^' class | alphanumeric '-' alphanumeric | alphanumeric+
// ASCII only.  Deviations from the reference's executor: repeat counts mean what they say,
// '/i' folds class members and range ends as well as literals, inputs the reference panics on or misparses are
// refused with a message, and a character class never contains byte 0 (a character never matches padding).
//
// Standard headers only: tests/regex_main.cpp links this file alone.
#pragma once
#include <stdint.h>

#include <bitset>
#include <string>
#include <vector>

namespace fhe {
namespace regex {

constexpr uint32_t kMaxPositions = 256;
constexpr uint32_t kUnbounded = 0xFFFFFFFFu;

typedef std::bitset<256> ByteSet;       // a character class; never contains byte 0
typedef std::bitset<kMaxPositions> PosSet;

struct Automaton {
    bool sof = false, eof = false;      // '^' / '$'
    bool nullable = false;              // the body matches the empty string
    std::vector<ByteSet> cls;           // [m]: class of position p (0-based)
    PosSet first, last;                 // positions a match may start / end with
    std::vector<PosSet> follow;         // [m]: follow[q] = positions that may come right after q
    uint32_t max_len = 0;               // longest match in characters; kUnbounded when there is none
    uint32_t positions() const { return (uint32_t)cls.size(); }
    // the body is one plain string (a chain of single-byte positions): its bytes, else empty
    std::string literal() const;
};

// 0 and `out`, or nonzero and the reason in `err` (a malformed pattern: with the byte offset).  Never throws on bad input.
int compile(const uint8_t* pattern, uint32_t len, Automaton& out, std::string& err);

}  // namespace regex
}  // namespace fhe
