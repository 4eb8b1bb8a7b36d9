// str_program.cpp -- the program builder and the layout table of the FheString plan names (see str_program.h).
// Standard headers only.
#include "str_program.h"

#include <atomic>

#include "str_op_name.h"

namespace fhe {
namespace program {

// The output layouts documented in include/fhestr.h, by plan name (str_op_name.h: the parsed name and its table row).
int op_layout(const std::string& op, uint32_t msg_mod, const uint32_t* caps, uint32_t n_caps, const uint8_t* clear,
              uint32_t clear_len, OpLayout& out, std::string& why) {
    out = OpLayout();
    const uint32_t bpc = opname::blocks_per_char(msg_mod);
    if (bpc == 0) {
        why = "string ops need msg_mod = 2^b with b | 8 and carry_mod >= msg_mod";
        return 1;
    }
    const opname::Name n = opname::parse(op);
    // no row, "bad numeric parameter", a matches without its clear pattern: the builder says what is wrong with the name
    if (n.status != opname::OK || (n.is(opname::MATCHES) && !n.clear)) {
        out.known = false;
        return 0;
    }
    const opname::Row& row = *n.row;
    const std::vector<uint32_t>& params = n.params;
    if (n.combines()) {
        // the shape is the name table's (opname::combine_shape); what it refuses, the builder refuses with the same words
        opname::Combine shape;
        uint32_t b_sum = 0;
        for (uint32_t i = 1; i < n_caps; i++) b_sum += caps[i];
        if (n.reference) out.refusal = "unknown string op: " + op;
        if (n.reference || opname::combine_shape(n, n_caps ? caps[0] : 0, b_sum, clear, clear_len, shape, out.refusal)) {
            out.known = false;
            return 0;
        }
        auto spec = [&](const opname::Piece& p) {
            const uint32_t blocks = p.kind == opname::A_STRING ? p.extent * bpc : p.kind == opname::A_COUNT ? opname::count_digits(msg_mod, p.extent) : 1;
            return ResultSpec{(Kind)p.kind, blocks, p.extent};
        };
        out.strings_min = out.strings_max = 0;
        for (const opname::Piece& p : shape.operands) {
            out.operands.push_back(spec(p));
            if (p.kind == opname::A_STRING) out.strings_min = ++out.strings_max;
        }
        for (const opname::Piece& p : shape.results) out.results.push_back(spec(p));
        return 0;
    }
    const bool full = params.size() == row.params;           // every parameter given (takes(): or none, or all but a part capacity)
    const uint64_t a_cap = n_caps ? caps[0] : 0;
    uint64_t b_cap = 0;
    for (uint32_t i = 1; i < n_caps; i++) b_cap += caps[i];

    auto bit = [&]() { out.results.push_back({BIT, 1, 1}); };
    auto count = [&](uint64_t n_max) { out.results.push_back({COUNT, opname::count_digits(msg_mod, n_max), (uint32_t)n_max}); };
    auto string = [&](uint64_t cap) { out.results.push_back({STRING, (uint32_t)(cap * bpc), (uint32_t)cap}); };

    // ---- operands ----
    if (row.unary() || n.clear || n.counted_repeat()) out.strings_min = out.strings_max = 1;
    else if (row.family == opname::REPLACE) {                                                   // a, from, to (no `to`: deletion)
        out.strings_min = 2;
        out.strings_max = 3;
        out.from_to = true;
        if (full) out.from_cap = params[params.size() - 2];
    }
    else out.strings_min = out.strings_max = 2;
    const bool counted = n.counted_repeat() || row.how == opname::COUNTED || row.split.enc_count;
    if (counted && !params.empty()) {
        out.takes_count = true;
        out.count_n_max = params[0];
        out.count_digits = opname::count_digits(msg_mod, params[0]);
        if (params[0] == 0) {                                // a bound of 0: "n_max must be at least 1", says the builder
            out.known = false;
            return 0;
        }
    }

    // ---- results (none where the builder will refuse: a missing parameter, a repeat_clear without its count) ----
    switch (row.family) {
    case opname::COMPARE: case opname::ORDER: case opname::AFFIX: case opname::IS_EMPTY: case opname::MATCHES:
        bit();
        break;
    case opname::FIND: bit(); count(a_cap); break;
    case opname::LEN: count(a_cap); break;
    case opname::STRIP_BIT: bit(); string(a_cap); break;
    case opname::UNARY_STRING: string(a_cap); break;
    case opname::CONCAT: string(a_cap + (n.clear ? clear_len : b_cap)); break;
    case opname::REPEAT:
        if (n.counted_repeat()) string(params[0] * a_cap);
        else if (n.clear && clear_len == 1 && clear && clear[0]) string((uint64_t)clear[0] * a_cap);
        break;
    case opname::REPLACE:
        if (row.takes(params.size())) string(full ? params.back() : a_cap);
        break;
    case opname::SPLIT:
        if (!row.takes(params.size())) break;
        if (row.split.once) {
            bit();
            for (int p = 0; p < 2; p++) string(full ? params[0] : a_cap);
        } else {
            const uint64_t P = params[0];
            count(P + 1);
            for (uint64_t p = 0; p < P && p < (1u << 16); p++) string(full ? params[1] : a_cap);
        }
        break;
    case opname::LOGIC: case opname::SELECT: case opname::COUNT: break;      // (answered above)
    case opname::SLICE:
        if (!row.takes(params.size()) || (n.clear && row.how != opname::INSERT)) break;
        if (row.how == opname::CHAR_AT) {
            bit();
            string(1);
        } else {
            const uint64_t cap = params.size() == 2 ? params[1] : a_cap + (row.how != opname::INSERT ? 0 : n.clear ? clear_len : b_cap);
            for (int p = 0; p < (row.how == opname::SPLIT_AT ? 2 : 1); p++) string(cap);
        }
        break;
    }
    return 0;
}

static const char* kind_name(Kind k) { return k == STRING ? "string" : k == BIT ? "bit" : "count"; }

// ids: [tag : 12][index : 20]
constexpr uint32_t INDEX_BITS = 20, INDEX_MASK = (1u << INDEX_BITS) - 1;

Program::Program(Backend& backend) : b_(backend) {
    static std::atomic<uint32_t> serial{0};
    tag_ = (serial.fetch_add(1) % 0xFFFu) + 1;
    b_.set_dedupe(true);
}

int Program::usable(std::string& why) const {
    if (finished_) { why = "string program: already finished (no declaration or op after finish)"; return 1; }
    if (!broken_.empty()) { why = "string program: unusable since an op was refused while it was being built: " + broken_; return 1; }
    return 0;
}

uint32_t Program::add_value(Kind kind, uint32_t extent, std::vector<uint32_t> nodes, uint32_t op_index) {
    values_.push_back({kind, extent, std::move(nodes), op_index});
    return (tag_ << INDEX_BITS) | (uint32_t)(values_.size() - 1);
}

int Program::set_dedupe(bool on, std::string& why) {
    if (usable(why)) return 1;
    b_.set_dedupe(on);
    return 0;
}

int Program::input_string(uint32_t cap, uint32_t& value, std::string& why) {
    if (usable(why)) return 1;
    if (cap == 0) { why = "string capacity must be > 0"; return 1; }
    const uint32_t M = b_.msg_modulus();
    const uint32_t bpc = opname::blocks_per_char(M);
    if (bpc == 0) { why = "string ops need msg_mod = 2^b with b | 8 and carry_mod >= msg_mod"; return 1; }
    if ((uint64_t)cap * bpc > INDEX_MASK || values_.size() >= INDEX_MASK) { why = "string program: too large"; return 1; }
    std::vector<uint32_t> nodes;
    for (uint32_t i = 0; i < cap * bpc; i++) nodes.push_back(b_.input(M - 1));
    value = add_value(STRING, cap, std::move(nodes), NO_OP);
    return 0;
}

int Program::input_count(uint32_t n_max, uint32_t& value, std::string& why) {
    if (usable(why)) return 1;
    if (n_max == 0) { why = "an encrypted count needs a bound n_max >= 1"; return 1; }
    if (values_.size() >= INDEX_MASK) { why = "string program: too large"; return 1; }
    const uint32_t M = b_.msg_modulus();
    std::vector<uint32_t> nodes;
    for (uint32_t i = 0; i < opname::count_digits(M, n_max); i++) nodes.push_back(b_.input(M - 1));
    value = add_value(COUNT, n_max, std::move(nodes), NO_OP);
    return 0;
}

int Program::input_bit(uint32_t& value, std::string& why) {
    if (usable(why)) return 1;
    if (values_.size() >= INDEX_MASK) { why = "string program: too large"; return 1; }
    value = add_value(BIT, 1, {b_.input(1)}, NO_OP);
    return 0;
}

int Program::value(uint32_t id, const Value*& v, std::string& why) const {
    v = nullptr;
    if ((id >> INDEX_BITS) != tag_) { why = "value " + std::to_string(id) + " belongs to another program"; return 1; }
    const uint32_t index = id & INDEX_MASK;
    if (index >= values_.size()) { why = "value " + std::to_string(id) + " is out of range: the program has " + std::to_string(values_.size()) + " values"; return 1; }
    v = &values_[index];
    return 0;
}

int Program::op(const std::string& name, const uint32_t* operands, uint32_t n_operands, const uint8_t* clear, uint32_t clear_len,
                uint32_t* results, uint32_t results_cap, uint32_t& n_results, std::string& why) {
    n_results = 0;
    if (usable(why)) return 1;
    if (n_operands && !operands) { why = "null pointer: operands"; return 1; }
    if (clear_len && !clear) { why = "null clear pattern"; return 1; }
    {
        const opname::Name parsed = opname::parse(name);
        if (parsed.status == opname::OK && parsed.combines()) {
            std::vector<const Value*> all;
            for (uint32_t i = 0; i < n_operands; i++) {
                const Value* v;
                if (value(operands[i], v, why)) { why = name + ": operand " + std::to_string(i) + ": " + why; return 1; }
                all.push_back(v);
            }
            return op_combined(name, all, clear, clear_len, results, results_cap, n_results, why);
        }
    }
    // operands: strings, then at most one count
    std::vector<const Value*> strings;
    const Value* count = nullptr;
    for (uint32_t i = 0; i < n_operands; i++) {
        const Value* v;
        if (value(operands[i], v, why)) { why = name + ": operand " + std::to_string(i) + ": " + why; return 1; }
        if (v->kind == STRING && !count) strings.push_back(v);
        else if (v->kind == COUNT && !count && i + 1 == n_operands) count = v;
        else {
            why = name + ": operand " + std::to_string(i) + " is a " + kind_name(v->kind) +
                  ": an op takes its strings, then at most one count as the last operand";
            return 1;
        }
    }
    if (strings.empty()) { why = name + ": the first operand must be a string"; return 1; }
    std::vector<uint32_t> caps;
    for (const Value* s : strings) caps.push_back(s->extent);
    OpLayout lay;
    if (op_layout(name, b_.msg_modulus(), caps.data(), (uint32_t)caps.size(), clear, clear_len, lay, why)) return 1;
    if (!lay.known) {
        // not a name of the layout table: the builder refuses it with its own message (what it would build could not be cut)
        lay.takes_count = count != nullptr;
        lay.count_digits = count ? (uint32_t)count->nodes.size() : 0;
        lay.from_to = false;
    } else if (strings.size() < lay.strings_min || strings.size() > lay.strings_max) {
        why = name + ": takes " + std::to_string(lay.strings_min) +
              (lay.strings_max != lay.strings_min ? " to " + std::to_string(lay.strings_max) : std::string()) +
              " encrypted string operand(s), got " + std::to_string(strings.size());
        return 1;
    }
    if (lay.known && lay.takes_count && !count) { why = name + ": takes an encrypted count as its last operand"; return 1; }
    if (!lay.takes_count && count) { why = name + ": takes no encrypted count"; return 1; }
    if (count && count->nodes.size() > lay.count_digits) {
        why = name + ": the count operand has " + std::to_string(count->nodes.size()) + " digits, the op takes " +
              std::to_string(lay.count_digits) + " (n_max = " + std::to_string(lay.count_n_max) + ")";
        return 1;
    }
    // the plan's single b operand of a replace form is from || to, cut where the name says
    if (lay.from_to) {
        const uint32_t to_cap = strings.size() == 3 ? strings[2]->extent : 0;
        if (lay.from_cap == 0 && strings[1]->extent != to_cap) {
            why = name + ": `from` and `to` of equal capacity (other shapes: replace:<from_cap>:<out_cap>)";
            return 1;
        }
        if (lay.from_cap && strings[1]->extent != lay.from_cap) {
            why = name + ": the name says a `from` of " + std::to_string(lay.from_cap) + " characters, the operand has " +
                  std::to_string(strings[1]->extent);
            return 1;
        }
    }
    n_results = (uint32_t)lay.results.size();
    if (results_fit(name, n_results, results, results_cap, why)) return 1;

    // the operands' nodes in the order the plan takes its inputs: string, pattern operand(s), count digits
    std::vector<uint32_t> queue;
    uint32_t b_cap = 0;
    for (size_t i = 0; i < strings.size(); i++) {
        queue.insert(queue.end(), strings[i]->nodes.begin(), strings[i]->nodes.end());
        if (i) b_cap += strings[i]->extent;
    }
    if (count) {
        queue.insert(queue.end(), count->nodes.begin(), count->nodes.end());
        for (size_t d = count->nodes.size(); d < lay.count_digits; d++) queue.push_back(b_.trivial(0));
    }
    return bind_and_build(name, lay.results, lay.known, queue, strings[0]->extent, b_cap, clear, clear_len, results, n_results, why);
}

int Program::results_fit(const std::string& name, uint32_t n, const uint32_t* results, uint32_t results_cap, std::string& why) const {
    if (n > results_cap) {
        why = name + ": results_cap " + std::to_string(results_cap) + " is too small, the op returns " + std::to_string(n) + " values";
        return 1;
    }
    if (n && !results) { why = "null pointer: results"; return 1; }
    if (values_.size() + n >= INDEX_MASK) { why = "string program: too large"; return 1; }
    return 0;
}

int Program::bind_and_build(const std::string& name, const std::vector<ResultSpec>& specs, bool known, const std::vector<uint32_t>& queue,
                            uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, uint32_t* results, uint32_t& n_results,
                            std::string& why) {
    const uint32_t mark = b_.n_outputs();
    b_.bind_inputs(queue);
    std::string refusal;
    const int rc = b_.build_op(name, a_cap, b_cap, clear, clear_len, refusal);
    const std::string bind_error = b_.end_binding();
    const std::vector<uint32_t> outs = b_.take_outputs(mark);
    if (rc || !bind_error.empty()) {
        why = rc ? refusal : "circuit build error: " + bind_error;
        broken_ = why;
        n_results = 0;
        return 1;
    }
    size_t total = 0;
    for (const ResultSpec& r : specs) total += r.blocks;
    if (total != outs.size() || !known) {
        why = known ? "internal: " + name + " declared " + std::to_string(outs.size()) + " outputs, its layout has " + std::to_string(total)
                    : name + ": not a name of the layout table of string programs, its outputs cannot be cut into values";
        broken_ = why;
        n_results = 0;
        return 1;
    }
    size_t at = 0;
    for (uint32_t i = 0; i < n_results; i++) {
        const ResultSpec& r = specs[i];
        results[i] = add_value(r.kind, r.extent, std::vector<uint32_t>(outs.begin() + at, outs.begin() + at + r.blocks), n_ops_);
        at += r.blocks;
    }
    n_ops_++;
    return 0;
}

// The names that combine results: bits and counts may come first; what the name takes is the name table's shape.  The
// capacities of a select's strings come from the operands.
int Program::op_combined(const std::string& name, const std::vector<const Value*>& operands, const uint8_t* clear, uint32_t clear_len,
                         uint32_t* results, uint32_t results_cap, uint32_t& n_results, std::string& why) {
    // the strings where the name may take them (a select: the first operand, and the second unless it is clear bytes)
    std::vector<uint32_t> caps;
    for (size_t i = 0; i < operands.size() && i < 2 && operands[i]->kind == STRING; i++) caps.push_back(operands[i]->extent);
    const opname::Name n = opname::parse(name);
    if (n.is(opname::SELECT) && n.row->how == opname::OF_STRINGS)
        caps.resize(n.clear ? 1 : 2, 1);                     // (a missing string: refused below, by its kind)
    else caps.clear();
    OpLayout lay;
    if (op_layout(name, b_.msg_modulus(), caps.data(), (uint32_t)caps.size(), clear, clear_len, lay, why)) return 1;
    if (!lay.known) {                                        // refused by the name alone: the circuit stays as it is
        why = lay.refusal;
        return 1;
    }
    std::string takes;
    for (const ResultSpec& o : lay.operands) takes += (takes.empty() ? "" : ", ") + std::string(kind_name(o.kind));
    if (operands.size() != lay.operands.size()) {
        why = name + ": takes " + std::to_string(lay.operands.size()) + " operand(s) (" + takes + "), got " + std::to_string(operands.size());
        return 1;
    }
    for (size_t i = 0; i < operands.size(); i++) {
        const Value& v = *operands[i];
        const ResultSpec& o = lay.operands[i];
        if (v.kind != o.kind) {
            why = name + ": operand " + std::to_string(i) + " is a " + kind_name(v.kind) + ": the op takes " + takes;
            return 1;
        }
        if (v.kind == COUNT && v.nodes.size() > o.blocks) {
            why = name + ": the count operand has " + std::to_string(v.nodes.size()) + " digits, the op takes " + std::to_string(o.blocks) +
                  " (n_max = " + std::to_string(o.extent) + ")";
            return 1;
        }
    }
    n_results = (uint32_t)lay.results.size();
    if (results_fit(name, n_results, results, results_cap, why)) return 1;
    std::vector<uint32_t> queue;
    for (size_t i = 0; i < operands.size(); i++) {
        queue.insert(queue.end(), operands[i]->nodes.begin(), operands[i]->nodes.end());
        for (size_t d = operands[i]->nodes.size(); d < lay.operands[i].blocks; d++) queue.push_back(b_.trivial(0));
    }
    return bind_and_build(name, lay.results, true, queue, caps.empty() ? 0 : caps[0], caps.size() > 1 ? caps[1] : 0, clear, clear_len, results,
                          n_results, why);
}

int Program::output(uint32_t id, std::string& why) {
    if (usable(why)) return 1;
    const Value* v;
    if (value(id, v, why)) return 1;
    for (uint32_t node : v->nodes) b_.output(node);
    outputs_.push_back(id);
    return 0;
}

int Program::can_finish(std::string& why) const {
    if (usable(why)) return 1;
    if (outputs_.empty()) { why = "string program: finish without outputs (declare them with output)"; return 1; }
    return 0;
}

int Program::finish(std::string& why) {
    if (can_finish(why)) return 1;
    finished_ = true;
    return 0;
}

}  // namespace program
}  // namespace fhe
