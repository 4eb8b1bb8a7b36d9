// str_slice.cpp -- StrOps: slicing at a clear or an encrypted position: take, skip, char_at, insert (str_ops.h; DESIGN.md
// section 3).  Python slicing on the unpadded bytes: positions beyond the hidden length clamp, an encrypted position above
// its public bound acts as the bound.
#include <algorithm>

#include "str_ops.h"

namespace fhe {

// The selectors of a barrel shifter by a number are the bits of that number.  Bit t of min(n, bound):
// one packed unit (D <= 2 digits): one lookup on the unit, the comparison with the bound inside the table.  More digits:
// [n >= bound] once (the thermometer's last entry), then one lookup per bit on (its digit) + M [n >= bound], which answers
// the bound's bit where the comparison is set.
std::vector<uint32_t> StrOps::count_bits(const std::vector<uint32_t>& digits, uint32_t bound) {
    uint32_t n_bits = 0;
    while (n_bits < 32 && (bound >> n_bits)) n_bits++;
    std::vector<uint32_t> bits;
    if (n_bits == 0) return bits;
    const bool pack = (uint64_t)M * M <= (uint64_t)T && 1.0 + (double)M * M <= budget();
    if (digits.size() <= (pack ? 2u : 1u)) {
        const uint32_t unit = digits.size() == 2 ? c.lin({{digits[0], 1}, {digits[1], (int32_t)M}}) : digits[0];
        for (uint32_t t = 0; t < n_bits; t++)
            bits.push_back(c.pbs(unit, c.lut_fn([bound, t](uint64_t x) { return (std::min<uint64_t>(x, bound) >> t) & 1; })));
        return bits;
    }
    const uint32_t ge = count_thermometer(digits, bound, bound)[0];
    const uint32_t mm = M;
    for (uint32_t t = 0; t < n_bits; t++) {
        const uint32_t digit = digits[t / bits_per_block], k = t % bits_per_block;
        const uint64_t of_bound = (bound >> t) & 1;
        if (2 * M <= T && c.node(digit).noise + (double)M * M * c.node(ge).noise <= budget()) {
            bits.push_back(c.pbs(c.lin({{digit, 1}, {ge, (int32_t)M}}), c.lut_fn([mm, k, of_bound](uint64_t x) { return x >= mm ? of_bound : (x >> k) & 1; })));
            continue;
        }
        const uint32_t raw = c.pbs(digit, c.lut_fn([mm, k](uint64_t x) { return ((x % mm) >> k) & 1; }));
        bits.push_back(c.pbs(c.lin({{raw, 1}, {ge, 2}}), c.lut_fn([of_bound](uint64_t x) { return x >= 2 ? of_bound : x & 1; })));
    }
    return bits;
}
// take: the keep mask [i < n] is the thermometer's g[i]; characters from min(cap, s.cap, n) on are known zeros.
Str StrOps::take(const Str& s, const Position& at, uint32_t cap) {
    const uint32_t kept = std::min({cap, s.cap, at.n});
    std::vector<uint32_t> g;
    if (at.enc() && kept) g = count_thermometer(*at.digits, kept);
    Str out = blank(kept);
    for (uint32_t i = 0; i < kept; i++) {
        Scope sc(c, owner_for(i, kept));
        for (uint32_t k = 0; k < bpc; k++) out.ch[i].push_back(at.enc() ? gate_block(s.ch[i][k], g[i], true) : s.ch[i][k]);
    }
    return out;
}
// skip: a barrel shifter whose stage t moves the string left by 2^t where bit t of the position is set.  Skipping s.cap
// characters and more leaves nothing, so the bits are those of min(n, n_max, s.cap): stages with 2^t above that do not exist.
Str StrOps::skip(const Str& s, const Position& at) {
    if (!at.enc()) {
        const uint32_t n = std::min(at.n, s.cap);
        Str out = blank(s.cap - n);
        for (uint32_t i = 0; i < out.cap; i++) out.ch[i].assign(s.ch[i + n].begin(), s.ch[i + n].begin() + bpc);
        return out;
    }
    const std::vector<uint32_t> bits = count_bits(*at.digits, std::min(at.n, s.cap));
    Str cur = fit(s, s.cap);
    for (size_t t = 0; t < bits.size(); t++) {
        const uint32_t sh = 1u << t;
        Str nxt = blank(s.cap);
        for (uint32_t i = 0; i < s.cap; i++) {
            Scope sc(c, owner_for(i, s.cap));
            for (uint32_t k = 0; k < bpc; k++)
                nxt.ch[i].push_back(i + sh < s.cap ? select_block(cur.ch[i][k], cur.ch[i + sh][k], bits[t], M - 1)
                                                   : gate_block(cur.ch[i][k], bits[t], false));
        }
        cur = nxt;
    }
    // blocks that went through select_block stages carry one nominal variance per stage: back to a fresh lookup's
    for (uint32_t i = 0; i < s.cap; i++) {
        Scope sc(c, owner_for(i, s.cap));
        for (uint32_t& b : cur.ch[i])
            if (c.node(b).noise > 2.0) b = fresh(b);
    }
    return cur;
}
// char_at: no shifter.  The one-hot [min(n, n_max) == i] = G(i) - G(i + 1) is linear in the thermometer (G(0) = 1,
// G(q) = 0 above the bound); every block is gated by its position's bit and the products are summed in groups the noise
// budget admits.  The valid bit [n < len(s)] is "the character is not NUL".
std::vector<uint32_t> StrOps::char_at(const Str& s, const Position& at) {
    std::vector<uint32_t> chr(bpc, c.trivial(0));
    if (!at.enc()) {
        if (at.n < s.cap) chr.assign(s.ch[at.n].begin(), s.ch[at.n].begin() + bpc);
    } else {
        const uint32_t last = std::min(s.cap - 1, at.n);              // the largest position that can be asked for
        const std::vector<uint32_t> g = count_thermometer(*at.digits, std::min(s.cap, at.n));
        auto G = [&](uint32_t q) { return q == 0 ? c.trivial(1) : q > g.size() ? c.trivial(0) : g[q - 1]; };
        std::vector<uint32_t> here;
        for (uint32_t i = 0; i <= last; i++) here.push_back(c.lin({{G(i), 1}, {G(i + 1), -1}}, 0, 1));
        for (uint32_t k = 0; k < bpc; k++) {
            std::vector<Term> terms;
            for (uint32_t i = 0; i <= last; i++) {
                Scope sc(c, owner_for(i, last + 1));
                terms.push_back({gate_block(s.ch[i][k], here[i], true), 1});
            }
            while (true) {
                const auto groups = term_groups(terms, SIZE_MAX);
                if (groups.size() <= 1) break;
                terms.clear();
                for (const auto& grp : groups) terms.push_back({fresh(c.lin(grp, 0, (int64_t)M - 1)), 1});
            }
            chr[k] = c.lin(terms, 0, (int64_t)M - 1);                 // (at most one term is not zero)
            if (c.node(chr[k]).noise > 2.0) chr[k] = fresh(chr[k]);
        }
    }
    std::vector<uint32_t> out{not_bit(char_is_zero(chr))};
    append(out, chr);
    return out;
}
// insert: s[:n], then t, then s[n:], joined by concat, which closes the hidden gaps of the pieces on its left.
Str StrOps::insert(const Str& s, const Position& at, const Operand& t, uint32_t cap) {
    Str r = take(s, at, s.cap);
    auto join = [&](const Str& piece) {
        if (piece.cap) r = r.cap ? concat(r, piece) : piece;
    };
    join(t.enc ? *t.enc : clear_string(t.bytes, t.len));
    join(skip(s, at));
    return fit(r, cap);
}
void StrOps::settle(std::vector<uint32_t>& blocks) {
    for (uint32_t& b : blocks)
        if (c.node(b).kind == Node::INPUT) b = c.pbs(b, lut_message());
}

}  // namespace fhe
