// Stand-alone driver of csrc/regex.cpp (the pattern parser and automaton construction of matches_clear): no engine, no
// device, standard headers only.  Prints one line per pattern,
//     <pattern, bytes outside 0x21..0x7e as \xNN> TAB ok TAB <positions> TAB <max_len | inf> TAB <literal or ->
//     <pattern>                                   TAB refused TAB <reason>
// for a valid corpus, malformed and truncated patterns, every prefix of a few valid patterns, deep nesting and huge
// repeat counts.  tests/test_regex_parser_host.py builds it with AddressSanitizer + UBSan and checks the table.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../fhe-string-bounty_amd/csrc/regex.h"

static std::string shown(const std::string& s) {
    std::string out;
    char buf[8];
    for (unsigned char ch : s) {
        if (ch > 0x20 && ch < 0x7f && ch != '\\') out.push_back((char)ch);
        else if (ch == '\\') out += "\\\\";
        else { snprintf(buf, sizeof buf, "\\x%02x", ch); out += buf; }
    }
    return out;
}

static int check_automaton(const fhe::regex::Automaton& g) {
    // what StrOps::matches relies on: consistent sizes, no byte 0 in any class, sets inside the positions
    const uint32_t m = g.positions();
    if (g.follow.size() != m || m > fhe::regex::kMaxPositions) return 1;
    for (uint32_t p = 0; p < m; p++)
        if (g.cls[p][0] || g.cls[p].none()) return 1;
    for (uint32_t p = m; p < fhe::regex::kMaxPositions; p++) {
        if (g.first[p] || g.last[p]) return 1;
        for (uint32_t q = 0; q < m; q++)
            if (g.follow[q][p]) return 1;
    }
    if (m && !g.nullable && (g.first.none() || g.last.none())) return 1;
    return 0;
}

static int report(const std::string& pattern) {
    fhe::regex::Automaton g;
    std::string err;
    const int rc = fhe::regex::compile(reinterpret_cast<const uint8_t*>(pattern.data()), (uint32_t)pattern.size(), g, err);
    if (rc) {
        if (err.empty()) return 1;
        printf("%s\trefused\t%s\n", shown(pattern).c_str(), err.c_str());
        return 0;
    }
    if (check_automaton(g)) return 1;
    const std::string lit = g.literal();
    const std::string len = g.max_len == fhe::regex::kUnbounded ? "inf" : std::to_string(g.max_len);
    printf("%s\tok\t%u\t%s\t%s\n", shown(pattern).c_str(), g.positions(), len.c_str(), lit.empty() ? "-" : shown(lit).c_str());
    return 0;
}

int main() {
    const std::vector<std::string> valid = {
        "/h/", "/&/", "/\\h/", "/./", "/abc/", "/^abc/", "/abc$/", "/^abc$/", "/^ab?c$/", "/^ab*c$/", "/^ab+c$/", "/^ab{2}c$/",
        "/^ab{3,}c$/", "/^ab{2,4}c$/", "/^ab{,4}c$/", "/^.$/", "/^[abc]$/", "/^[a-d]$/", "/^[^abc]$/", "/^[^a-d]$/", "/^abc$/i",
        "/^a(bc)d$/", "/ab|cd/", "/^ab|cd|de$/", "/^[0-9]*$/", "/[a-z]+@[a-z]+/", "/ab|cd/i", "/[a-c]/i", "/\\//", "/\\\\/",
        "/^$/", "/^/", "/$/", "/a{0}/", "/a{,}/", "/(a{0}){999999999}/", "/(a|b)*abb/", "/((a|b)?c){2,3}$/", "/[^^a]/",
        "/(a{16}){16}/", "/a{256}/", "/(a?){256}/", "/x(a|b|c|d|e|f|g|h|i|j)k/",
    };
    const std::vector<std::string> malformed = {
        "", "/", "//", "a", "/a", "/a/x", "/a/ii", "/a**/", "/*a/", "/+/", "/?/", "/{2}/", "/a{}/", "/a{3,2}/", "/a{2/", "/a{2,/", "/a{x}/",
        "/a{2,3,4}/", "/a|/", "/|a/", "/a||b/", "/()/", "/(|a)/", "/(a/", "/a)/", "/)/", "/[/", "/[]/", "/[a/", "/[a-]/", "/[-a]/", "/[a-zA]/",
        "/[z-a]/", "/[^]/", "/[a.]/", "/\\", "/a\\", "/a$b/", "/a^b/", "/^^a/", "/a$$/", "/a b/", "/a=b/", "/<a>/", "/a{999999999}/",
        "/a{99999999999999999999}/", "/a{257}/", "/(a{16}){17}/", "/((a{200}){200}){200}/", "/(a+){300}/", "/a{1,999999999}/",
        std::string("/a\0b/", 5), "/caf\xc3\xa9/", "/\xff/", "/[\x80]/", "/\\\xe9/",
    };
    int bad = 0;
    for (const auto& p : valid) bad |= report(p);
    for (const auto& p : malformed) bad |= report(p);
    // every prefix of a few valid patterns (truncation anywhere must be refused or accepted, never crash)
    for (const char* full : {"/^(ab|c[d-f]+){2,3}\\.x*$/i", "/[^a-c]?(x|yz{,2})+@[0-9]{2}/", "/((a|b)(c|d)){2}e{1,}/"})
        for (size_t n = 0; n <= strlen(full); n++) bad |= report(std::string(full, n));
    // deep nesting: accepted up to the limit, refused beyond it, unbalanced either way
    for (int depth : {1, 8, 64, 65, 1000, 100000}) {
        bad |= report("/" + std::string(depth, '(') + "a" + std::string(depth, ')') + "/");
        bad |= report("/" + std::string(depth, '(') + "a/");
        bad |= report("/a" + std::string(depth, ')') + "/");
    }
    // long patterns: 256 literal characters fit, 257 do not; a long alternation; repeats of repeats
    bad |= report("/" + std::string(256, 'a') + "/");
    bad |= report("/" + std::string(257, 'a') + "/");
    {
        std::string alt = "/a";
        for (int i = 0; i < 255; i++) alt += "|a";
        bad |= report(alt + "/");
        bad |= report(alt + "|a/");
    }
    // the null pointer with a length, and with none
    {
        fhe::regex::Automaton g;
        std::string err;
        if (!fhe::regex::compile(nullptr, 3, g, err) || err.empty()) bad = 1;
        if (!fhe::regex::compile(nullptr, 0, g, err) || err.empty()) bad = 1;
    }
    return bad;
}
