// regex.cpp -- recursive-descent parser of the reference's pattern text and the Glushkov construction (see regex.h).
#include "regex.h"

#include <algorithm>

namespace fhe {
namespace regex {
namespace {

constexpr uint64_t kInf = ~0ull;
constexpr uint32_t kNoMax = 0xFFFFFFFFu;       // '{n,}'
constexpr uint32_t kMaxDepth = 64;             // nested groups: the parser and the construction recurse once per level
constexpr uint64_t kCountCap = 1ull << 32;     // saturation of position counts and repeat bounds

struct AstNode {
    enum Kind : uint8_t { CHAR, CAT, ALT, REP } kind = CHAR;
    std::vector<uint32_t> kids;    // CAT / ALT: the parts; REP: one
    uint32_t lo = 0, hi = 0;       // REP: hi == kNoMax: no upper bound
    ByteSet set;                   // CHAR: the members as written
    bool negated = false;          // CHAR: [^...]
};

bool is_alnum(uint8_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
bool is_plain_symbol(uint8_t c) {
    for (const char* s = "&;:,`~-_!@#%'\""; *s; s++)
        if ((uint8_t)*s == c) return true;
    return false;
}

struct Parser {
    const uint8_t* s;
    uint32_t n, pos = 0, depth = 0;
    std::vector<AstNode> nodes;
    std::string err;

    Parser(const uint8_t* s, uint32_t n) : s(s), n(n) {}
    bool at_end() const { return pos >= n; }
    uint8_t peek() const { return s[pos]; }
    bool fail_at(uint32_t where, const std::string& why) {
        if (err.empty()) err = "malformed pattern at byte " + std::to_string(where) + ": " + why;
        return false;
    }
    uint32_t add(const AstNode& node) { nodes.push_back(node); return (uint32_t)nodes.size() - 1; }
    bool atom_starts() const {
        if (at_end()) return false;
        const uint8_t c = peek();
        return c == '.' || c == '\\' || c == '[' || c == '(' || is_alnum(c) || is_plain_symbol(c);
    }

    // regex = term ('|' regex)?     `what`: how an empty alternative is named here
    bool regex(uint32_t& out, const char* what) {
        AstNode alt;
        alt.kind = AstNode::ALT;
        for (;;) {
            uint32_t t;
            if (!term(t, alt.kids.empty() && (at_end() || peek() != '|') ? what : "empty alternative")) return false;
            alt.kids.push_back(t);
            if (at_end() || peek() != '|') break;
            pos++;
        }
        out = alt.kids.size() == 1 ? alt.kids[0] : add(alt);
        return true;
    }
    bool term(uint32_t& out, const char* what_if_empty) {
        AstNode cat;
        cat.kind = AstNode::CAT;
        while (atom_starts()) {
            uint32_t f;
            if (!factor(f)) return false;
            cat.kids.push_back(f);
        }
        if (cat.kids.empty()) {
            if (at_end()) return fail_at(pos, "unexpected end of the pattern");
            const uint8_t c = peek();
            if (c == '?' || c == '*' || c == '+' || c == '{') return fail_at(pos, "a repeat with nothing to repeat");
            if (c == ')' && depth == 0) return fail_at(pos, "unbalanced )");
            if (c == '|' || c == ')' || c == '/' || c == '$') return fail_at(pos, what_if_empty);
            return fail_at(pos, "unexpected byte");
        }
        out = cat.kids.size() == 1 ? cat.kids[0] : add(cat);
        return true;
    }
    bool number(uint32_t& value, bool& present) {
        uint64_t v = 0;
        present = false;
        while (!at_end() && peek() >= '0' && peek() <= '9') {
            v = std::min<uint64_t>(v * 10 + (peek() - '0'), kCountCap);
            present = true;
            pos++;
        }
        value = (uint32_t)std::min<uint64_t>(v, kNoMax - 1);
        return true;
    }
    bool factor(uint32_t& out) {
        uint32_t a;
        if (!atom(a)) return false;
        out = a;
        if (at_end()) return true;
        AstNode rep;
        rep.kind = AstNode::REP;
        rep.kids.push_back(a);
        const uint8_t q = peek();
        if (q == '?') { rep.lo = 0; rep.hi = 1; pos++; }
        else if (q == '*') { rep.lo = 0; rep.hi = kNoMax; pos++; }
        else if (q == '+') { rep.lo = 1; rep.hi = kNoMax; pos++; }
        else if (q == '{') {
            const uint32_t open = pos++;
            bool has_lo = false, has_hi = false, comma = false;
            uint32_t lo = 0, hi = 0;
            number(lo, has_lo);
            if (!at_end() && peek() == ',') { comma = true; pos++; number(hi, has_hi); }
            if (at_end()) return fail_at(pos, "unterminated repeat count");
            if (peek() != '}') return fail_at(pos, "unexpected byte in a repeat count");
            pos++;
            if (!has_lo && !comma) return fail_at(open, "empty repeat count {}");
            rep.lo = has_lo ? lo : 0;
            rep.hi = comma ? (has_hi ? hi : kNoMax) : lo;
            if (rep.hi != kNoMax && rep.lo > rep.hi) return fail_at(open, "repeat count {n,m} with n > m");
        } else {
            return true;
        }
        out = add(rep);
        return true;
    }
    bool atom(uint32_t& out) {
        const uint32_t start = pos;
        const uint8_t c = s[pos++];
        AstNode ch;
        if (c == '.') {
            ch.set.set();
        } else if (c == '\\') {
            if (at_end()) return fail_at(start, "escape at the end of the pattern");
            ch.set.set(s[pos++]);
        } else if (c == '(') {
            if (++depth > kMaxDepth) return fail_at(start, "groups nested too deeply");
            if (!regex(out, "empty group")) return false;
            if (at_end() || peek() != ')') return fail_at(pos, at_end() ? "unterminated group" : "unexpected byte in a group");
            pos++;
            depth--;
            return true;
        } else if (c == '[') {
            while (!at_end() && peek() == '^') { ch.negated = !ch.negated; pos++; }
            if (pos + 2 < n && is_alnum(s[pos]) && s[pos + 1] == '-' && is_alnum(s[pos + 2])) {
                if (s[pos] > s[pos + 2]) return fail_at(pos, "class range out of order");
                for (uint32_t v = s[pos]; v <= s[pos + 2]; v++) ch.set.set(v);
                pos += 3;
            } else {
                if (at_end()) return fail_at(pos, "unterminated class");
                if (!is_alnum(peek())) return fail_at(pos, peek() == ']' ? "empty class" : "a class holds alphanumerics or one range x-y");
                while (!at_end() && is_alnum(peek())) ch.set.set(s[pos++]);
            }
            if (at_end()) return fail_at(pos, "unterminated class");
            if (peek() != ']') return fail_at(pos, "a class holds alphanumerics or one range x-y");
            pos++;
        } else {
            ch.set.set(c);       // alphanumeric or plain symbol (atom_starts)
        }
        out = add(ch);
        return true;
    }
};

struct Frag {
    bool nullable = true;
    PosSet first, last;
    uint64_t max_len = 0;
};

struct Builder {
    const std::vector<AstNode>& nodes;
    bool icase;
    Automaton& g;
    std::vector<uint64_t> count_memo;

    Builder(const std::vector<AstNode>& nodes, bool icase, Automaton& g) : nodes(nodes), icase(icase), g(g), count_memo(nodes.size(), kInf) {}

    // positions the node expands to (saturating)
    uint64_t count(uint32_t id) {
        if (count_memo[id] != kInf) return count_memo[id];
        const AstNode& nd = nodes[id];
        uint64_t c = 0;
        if (nd.kind == AstNode::CHAR) c = 1;
        else if (nd.kind == AstNode::REP) {
            const uint64_t copies = nd.hi == kNoMax ? std::max<uint32_t>(nd.lo, 1) : nd.hi;
            c = std::min(count(nd.kids[0]) * copies, kCountCap);      // both factors <= 2^32
        } else {
            for (uint32_t k : nd.kids) c = std::min(c + count(k), kCountCap);
        }
        return count_memo[id] = c;
    }
    static uint64_t add_len(uint64_t a, uint64_t b) { return a == kInf || b == kInf ? kInf : a + b; }
    Frag cat(const Frag& a, const Frag& b) {
        for (uint32_t q = 0; q < g.positions(); q++)
            if (a.last[q]) g.follow[q] |= b.first;
        Frag r;
        r.nullable = a.nullable && b.nullable;
        r.first = a.nullable ? a.first | b.first : a.first;
        r.last = b.nullable ? a.last | b.last : b.last;
        r.max_len = add_len(a.max_len, b.max_len);
        return r;
    }
    void loop(Frag& f) {
        for (uint32_t q = 0; q < g.positions(); q++)
            if (f.last[q]) g.follow[q] |= f.first;
        if (f.first.any()) f.max_len = kInf;
    }
    Frag build(uint32_t id) {
        const AstNode& nd = nodes[id];
        Frag r;
        if (nd.kind == AstNode::CHAR) {
            ByteSet set = nd.set;
            if (icase)
                for (uint32_t v = 'a'; v <= 'z'; v++) {
                    const bool either = nd.set[v] || nd.set[v - 32];
                    set[v] = either;
                    set[v - 32] = either;
                }
            if (nd.negated) set.flip();
            set.reset(0);                                  // a character never matches padding
            const uint32_t p = g.positions();
            g.cls.push_back(set);
            g.follow.emplace_back();
            r.nullable = false;
            r.first.set(p);
            r.last.set(p);
            r.max_len = 1;
        } else if (nd.kind == AstNode::CAT) {
            for (uint32_t k : nd.kids) r = cat(r, build(k));
        } else if (nd.kind == AstNode::ALT) {
            r.nullable = false;
            for (uint32_t k : nd.kids) {
                const Frag f = build(k);
                r.nullable = r.nullable || f.nullable;
                r.first |= f.first;
                r.last |= f.last;
                r.max_len = f.max_len == kInf || r.max_len == kInf ? kInf : std::max(r.max_len, f.max_len);
            }
        } else {
            const uint32_t a = nd.kids[0];
            if (count(a) == 0) return r;                   // nothing to repeat: the empty string
            // lo copies in a row (the last one looped when there is no upper bound), then hi - lo nested optional ones
            for (uint32_t k = 0; k < nd.lo; k++) {
                Frag f = build(a);
                if (nd.hi == kNoMax && k + 1 == nd.lo) loop(f);
                r = cat(r, f);
            }
            if (nd.hi == kNoMax && nd.lo == 0) {
                Frag f = build(a);
                loop(f);
                f.nullable = true;
                r = cat(r, f);
            } else if (nd.hi != kNoMax && nd.hi > nd.lo) {
                Frag tail;
                for (uint32_t k = nd.lo; k < nd.hi; k++) {
                    tail = cat(build(a), tail);
                    tail.nullable = true;
                }
                r = cat(r, tail);
            }
        }
        return r;
    }
};

}  // namespace

std::string Automaton::literal() const {
    const uint32_t m = positions();
    std::string out;
    if (m == 0 || nullable || first.count() != 1 || !first[0] || last.count() != 1 || !last[m - 1]) return out;
    for (uint32_t q = 0; q < m; q++) {
        if (cls[q].count() != 1) return std::string();
        if (q + 1 < m ? (follow[q].count() != 1 || !follow[q][q + 1]) : follow[q].any()) return std::string();
    }
    for (uint32_t q = 0; q < m; q++)
        for (uint32_t v = 1; v < 256; v++)
            if (cls[q][v]) out.push_back((char)v);
    return out;
}

int compile(const uint8_t* pattern, uint32_t len, Automaton& out, std::string& err) {
    out = Automaton();
    err.clear();
    if (!pattern && len) { err = "null pattern"; return 1; }
    for (uint32_t i = 0; i < len; i++) {
        if (pattern[i] >= 0x80) { err = "non-ASCII byte at offset " + std::to_string(i) + ": patterns are ASCII only"; return 1; }
        if (pattern[i] == 0) { err = "malformed pattern at byte " + std::to_string(i) + ": a NUL byte (it would match the padding)"; return 1; }
    }
    Parser ps(pattern, len);
    auto bad = [&](uint32_t where, const char* why) { ps.fail_at(where, why); err = ps.err; return 1; };
    if (len == 0 || pattern[0] != '/') return bad(0, "a pattern is written /.../ or /.../i");
    ps.pos = 1;
    if (!ps.at_end() && ps.peek() == '^') { out.sof = true; ps.pos++; }
    uint32_t root = 0;
    // an anchored pattern may have no body (/^$/ is the empty string); // is refused
    const bool has_body = !ps.at_end() && ps.peek() != '$' && ps.peek() != '/';
    if (!has_body && !out.sof && (ps.at_end() || ps.peek() != '$')) return bad(ps.pos, ps.at_end() ? "missing the closing /" : "empty pattern");
    if (has_body && !ps.regex(root, "empty pattern")) { err = ps.err; return 1; }
    if (!ps.at_end() && ps.peek() == '$') { out.eof = true; ps.pos++; }
    if (ps.at_end()) return bad(ps.pos, "missing the closing /");
    if (ps.peek() != '/') return bad(ps.pos, ps.peek() == ')' ? "unbalanced )" : "unexpected byte");
    ps.pos++;
    bool icase = false;
    if (!ps.at_end() && ps.peek() == 'i') { icase = true; ps.pos++; }
    if (!ps.at_end()) return bad(ps.pos, "unexpected byte after the closing /");
    if (!has_body) {
        out.nullable = true;
        return 0;
    }
    Builder b(ps.nodes, icase, out);
    if (b.count(root) > kMaxPositions) {
        out = Automaton();
        err = "pattern expands to more than 256 automaton positions";
        return 1;
    }
    const Frag f = b.build(root);
    out.nullable = f.nullable;
    out.first = f.first;
    out.last = f.last;
    out.max_len = f.max_len == kInf ? kUnbounded : (uint32_t)f.max_len;
    return 0;
}

}  // namespace regex
}  // namespace fhe
