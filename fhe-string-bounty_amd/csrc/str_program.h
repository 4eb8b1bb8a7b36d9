// str_program.h -- string programs: several FheString operations recorded into ONE circuit.
//
// Every operation of fhe_string.cpp is a plan of its own (build_string_op).  A program binds the inputs of an operation
// to nodes that already exist in its circuit -- program inputs or the results of earlier operations (Circuit::bind_inputs)
// -- and turns the operation's outputs into values instead of plan outputs (Circuit::take_outputs).  Independent
// operations then share lookup levels (depth = the maximum, not the sum), and with hash-consing (Circuit::set_dedupe, on
// by default here) identical sub-circuits -- a match vector, compare_sign, the case fold -- are built once.
//
// This file and str_program.cpp use standard headers only: the circuit is reached through `Backend`, which c_api.cpp
// implements over Circuit + build_string_op and tests/str_program_main.cpp over a recorder.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace fhe {
namespace program {

enum Kind : uint32_t { STRING = 0, BIT = 1, COUNT = 2 };

// One result of an operation: `blocks` output ciphertexts; extent = the capacity in characters (STRING), the public
// bound n_max (COUNT: blocks = the smallest D with msg_mod^D > n_max little-endian digits) or 1 (BIT).
struct ResultSpec {
    Kind kind;
    uint32_t blocks, extent;
};

// What a plan name takes and returns (include/fhestr.h, "string programs": the layout table).
struct OpLayout {
    bool known = true;                           // false: not a name of the table (no operand rule, no results)
    uint32_t strings_min = 1, strings_max = 1;   // encrypted string operands: a, then the pattern operand(s)
    bool takes_count = false;                    // then the digits of an encrypted count, the plan's last inputs
    uint32_t count_n_max = 0, count_digits = 0;
    bool from_to = false;                        // the replace forms: the operands after a are `from` and `to` ...
    uint32_t from_cap = 0;                       // ... of these many characters (0: equal capacities)
    std::vector<ResultSpec> results;             // in output order
    // The names that combine results (bit logic, select, count arithmetic) take bits and counts as well as strings: their
    // operands in input order, a condition bit last.  Empty for every other name: the string rule above holds.
    std::vector<ResultSpec> operands;
    std::string refusal;                         // a combining name that is not known: why its shape is refused, in the builder's words
};

// 0, or nonzero with the reason in `why`.  caps: the capacities of the encrypted string operands as given (a first); for a
// name that combines results those of its string operands, none for one that takes bits and counts only.
// Refused here: a msg_mod no string operation works on.  A name the table does not know or cannot parse (known = false),
// and one it knows but the builder refuses (a missing parameter, a malformed regular expression: no results), are left
// to build_string_op, which says why.
int op_layout(const std::string& op, uint32_t msg_mod, const uint32_t* caps, uint32_t n_caps, const uint8_t* clear,
              uint32_t clear_len, OpLayout& out, std::string& why);

struct Backend {
    virtual ~Backend() {}
    virtual uint32_t msg_modulus() const = 0;
    virtual uint32_t input(uint64_t degree) = 0;
    virtual uint32_t trivial(int64_t value) = 0;
    virtual void set_dedupe(bool on) = 0;
    virtual void bind_inputs(const std::vector<uint32_t>& nodes) = 0;
    virtual std::string end_binding() = 0;                    // the circuit's build error, empty when there is none
    virtual uint32_t n_outputs() const = 0;
    virtual std::vector<uint32_t> take_outputs(uint32_t mark) = 0;
    virtual void output(uint32_t node) = 0;
    // build_string_op on the circuit; nonzero: refused, the reason in `why`
    virtual int build_op(const std::string& op, uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len,
                         std::string& why) = 0;
};

struct Value {
    Kind kind;
    uint32_t extent;               // capacity (STRING), n_max (COUNT), 1 (BIT)
    std::vector<uint32_t> nodes;   // one per block
    uint32_t op_index;             // the op that produced it; NO_OP for a program input
};
constexpr uint32_t NO_OP = 0xFFFFFFFFu;

class Program {
public:
    explicit Program(Backend& backend);
    // every call: 0, or nonzero with the reason in `why`
    int set_dedupe(bool on, std::string& why);
    int input_string(uint32_t cap, uint32_t& value, std::string& why);
    int input_count(uint32_t n_max, uint32_t& value, std::string& why);
    int input_bit(uint32_t& value, std::string& why);
    // `n_results` is set as soon as the layout is known, also when results_cap is too small (nothing is built then)
    int op(const std::string& name, const uint32_t* operands, uint32_t n_operands, const uint8_t* clear, uint32_t clear_len,
           uint32_t* results, uint32_t results_cap, uint32_t& n_results, std::string& why);
    int value(uint32_t id, const Value*& v, std::string& why) const;
    int output(uint32_t id, std::string& why);
    int can_finish(std::string& why) const;
    int finish(std::string& why);
    bool finished() const { return finished_; }
    uint32_t n_ops() const { return n_ops_; }
    const std::vector<uint32_t>& outputs() const { return outputs_; }     // value ids, in output order

private:
    uint32_t add_value(Kind kind, uint32_t extent, std::vector<uint32_t> nodes, uint32_t op_index);
    int usable(std::string& why) const;
    int op_combined(const std::string& name, const std::vector<const Value*>& operands, const uint8_t* clear, uint32_t clear_len,
                    uint32_t* results, uint32_t results_cap, uint32_t& n_results, std::string& why);
    int results_fit(const std::string& name, uint32_t n, const uint32_t* results, uint32_t results_cap, std::string& why) const;
    // binds `queue` to the inputs of `name`, builds it and cuts its outputs into the values of `specs`
    int bind_and_build(const std::string& name, const std::vector<ResultSpec>& specs, bool known, const std::vector<uint32_t>& queue,
                       uint32_t a_cap, uint32_t b_cap, const uint8_t* clear, uint32_t clear_len, uint32_t* results, uint32_t& n_results,
                       std::string& why);
    Backend& b_;
    uint32_t tag_;                 // value ids carry it: an id of another program is recognised
    std::vector<Value> values_;
    std::vector<uint32_t> outputs_;
    uint32_t n_ops_ = 0;
    bool finished_ = false;
    std::string broken_;           // the refusal that left half an operation in the circuit
};

}  // namespace program
}  // namespace fhe
