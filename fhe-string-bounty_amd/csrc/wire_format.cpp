// wire_format.cpp -- tfhe-rs 0.5 serialized forms of the objects either side of the hot path, so that a
// real tfhe-rs client can hand ciphertexts and server keys to the engine and read results back.
//
// The reference serializes with serde + bincode 1.x: `bincode::serialize` (legacy config) and
// `safe_serialize` (DefaultOptions + with_fixint_encoding, safe_deserialization.rs:30-99) agree on these
// types: little endian, fixed-width integers, usize as u64, u128 as 16 bytes, Vec<T> / String as a u64
// length then the elements, structs as their fields in declaration order, a unit enum variant as its u32
// index.  Field orders are those of the struct definitions:
//   LweCiphertext<Vec<u64>>      { data, ciphertext_modulus }                          entities/lwe_ciphertext.rs:500-507
//   LweKeyswitchKey<Vec<u64>>    { data, decomp_base_log, decomp_level_count, output_lwe_size,
//                                  ciphertext_modulus }                                entities/lwe_keyswitch_key.rs:76-86
//   LweBootstrapKey<Vec<u64>>    { ggsw_list: GgswCiphertextList { data, glwe_size, polynomial_size,
//                                  decomp_base_log, decomp_level_count, ciphertext_modulus } }
//                                                     entities/lwe_bootstrap_key.rs:98-106, ggsw_ciphertext_list.rs:9-20
//   CiphertextModulus<u64>       { modulus: u128 (0 = native 2^64), scalar_bits: usize }
//                                                     commons/ciphertext_modulus.rs:41-64
//   shortint::Ciphertext         { ct, degree, noise_level, message_modulus, carry_modulus, pbs_order }
//                                                     shortint/ciphertext/mod.rs:261-270 (all usize newtypes; PBSOrder:
//                                                     commons/parameters.rs:233-245)
//   safe_serialize framing       String "0.1", String T::NAME ("shortint::Ciphertext"), then the object, each
//                                under its own size limit                              safe_deserialization.rs:16-54
// The data layouts inside `data` are the flat layouts the C ABI already uses (fhestr.h).
// The reference ships no serialized fixture and cannot be run here: byte-level PARITY IS UNPINNED; the
// tests pin the layout against the bincode rules above on hand-built examples and round trips.
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "glwe_narrow.h"

namespace {

using fhe::fail;

struct Writer {
    uint8_t* out;
    size_t cap, pos = 0;
    bool overflow = false;
    void bytes(const void* p, size_t n) {
        if (out) {
            if (pos + n > cap) overflow = true;
            else std::memcpy(out + pos, p, n);
        }
        pos += n;
    }
    void u32(uint32_t v) { uint8_t b[4]; for (int i = 0; i < 4; i++) b[i] = (uint8_t)(v >> (8 * i)); bytes(b, 4); }
    void u64(uint64_t v) { uint8_t b[8]; for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i)); bytes(b, 8); }
    void vec_u64(const uint64_t* v, size_t n) {
        u64(n);
        if (out && pos + n * 8 <= cap) {            // little-endian host: one copy
            std::memcpy(out + pos, v, n * 8);
            pos += n * 8;
        } else {
            if (out) overflow = true;
            pos += n * 8;
        }
    }
    void str(const char* s) { const size_t n = std::strlen(s); u64(n); bytes(s, n); }
    void native_modulus_u64() { u64(0); u64(0); u64(64); }   // u128 0 = native, scalar_bits = 64
};

struct Reader {
    const uint8_t* in;
    size_t len, pos = 0;
    std::string err;
    bool need(size_t n) {
        if (!err.empty()) return false;
        if (n > len - pos) { err = "truncated input"; return false; }
        return true;
    }
    uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)in[pos + i] << (8 * i); pos += 4; return v; }
    uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)in[pos + i] << (8 * i); pos += 8; return v; }
    // Vec<u64> of exactly / at most `max_words` into dst; returns the element count
    size_t vec_u64(uint64_t* dst, size_t max_words) {
        const uint64_t n = u64();
        if (!err.empty()) return 0;
        if (n > max_words) { err = "vector longer than the destination (" + std::to_string(n) + " words)"; return 0; }
        if (n > (len - pos) / 8) { err = "truncated input"; return 0; }
        std::memcpy(dst, in + pos, (size_t)n * 8);
        pos += (size_t)n * 8;
        return (size_t)n;
    }
    std::string str(uint64_t limit) {
        const uint64_t n = u64();
        if (!err.empty()) return "";
        if (n > limit) { err = "string longer than its size limit"; return ""; }
        if (!need((size_t)n)) return "";
        std::string s(reinterpret_cast<const char*>(in + pos), (size_t)n);
        pos += (size_t)n;
        return s;
    }
    void native_modulus_u64() {
        const uint64_t lo = u64(), hi = u64(), bits = u64();
        if (!err.empty()) return;
        if (bits != 64) err = "expected an unsigned integer with 64 bits, got " + std::to_string(bits);   // ciphertext_modulus.rs:74-80
        else if (lo != 0 || hi != 0) err = "only the native modulus 2^64 is supported";
    }
};

int finish(Writer& w, size_t* written) {
    if (written) *written = w.pos;
    if (w.overflow) return fail("output buffer too small: " + std::to_string(w.pos) + " bytes needed");
    return 0;
}

constexpr const char* kVersion = "0.1";                     // safe_deserialization.rs:16
constexpr const char* kShortintName = "shortint::Ciphertext";   // shortint/ciphertext/mod.rs:272-274

}  // namespace

extern "C" {

int fhe_wire_write_lwe_ciphertext(const uint64_t* ct, size_t lwe_size, uint8_t* out, size_t out_cap, size_t* written) {
    if (!ct || lwe_size == 0) return fail("null / empty ciphertext");
    Writer w{out, out_cap};
    w.vec_u64(ct, lwe_size);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_lwe_ciphertext(const uint8_t* in, size_t in_len, uint64_t* ct, size_t ct_cap, size_t* lwe_size,
                                 size_t* consumed) {
    if (!in || !ct) return fail("null pointer");
    Reader r{in, in_len};
    const size_t n = r.vec_u64(ct, ct_cap);
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("LweCiphertext: " + r.err);
    if (n == 0) return fail("LweCiphertext: empty container");
    if (lwe_size) *lwe_size = n;
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_keyswitch_key(const fhe_params_t* p, const uint64_t* ksk, uint8_t* out, size_t out_cap, size_t* written) {
    if (!p || !ksk) return fail("null pointer");
    Writer w{out, out_cap};
    w.vec_u64(ksk, (size_t)p->k * p->N * p->ks_level * (p->n + 1));
    w.u64(p->ks_base_log);
    w.u64(p->ks_level);
    w.u64((uint64_t)p->n + 1);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_keyswitch_key(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* ksk, size_t* consumed) {
    if (!p || !in || !ksk) return fail("null pointer");
    const size_t want = (size_t)p->k * p->N * p->ks_level * (p->n + 1);
    Reader r{in, in_len};
    const size_t n = r.vec_u64(ksk, want);
    const uint64_t base_log = r.u64(), level = r.u64(), out_size = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("LweKeyswitchKey: " + r.err);
    // ParameterSetConformant-style checks (conformance.rs): every dimension must be the parameter set's
    if (base_log != p->ks_base_log || level != p->ks_level || out_size != (uint64_t)p->n + 1 || n != want)
        return fail("LweKeyswitchKey does not match the parameter set (base_log " + std::to_string(base_log) + ", level " +
                    std::to_string(level) + ", output size " + std::to_string(out_size) + ", " + std::to_string(n) + " words)");
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_bootstrap_key(const fhe_params_t* p, const uint64_t* bsk_std, uint8_t* out, size_t out_cap, size_t* written) {
    if (!p || !bsk_std) return fail("null pointer");
    if (p->grouping_factor > 1) return fail("multi-bit bootstrap keys have their own container: use fhe_wire_{read,write}_multi_bit_bootstrap_key");
    Writer w{out, out_cap};
    w.vec_u64(bsk_std, (size_t)p->n * p->pbs_level * (p->k + 1) * (p->k + 1) * p->N);
    w.u64((uint64_t)p->k + 1);
    w.u64(p->N);
    w.u64(p->pbs_base_log);
    w.u64(p->pbs_level);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_bootstrap_key(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* bsk_std, size_t* consumed) {
    if (!p || !in || !bsk_std) return fail("null pointer");
    if (p->grouping_factor > 1) return fail("multi-bit bootstrap keys have their own container: use fhe_wire_{read,write}_multi_bit_bootstrap_key");
    const size_t want = (size_t)p->n * p->pbs_level * (p->k + 1) * (p->k + 1) * p->N;
    Reader r{in, in_len};
    const size_t n = r.vec_u64(bsk_std, want);
    const uint64_t glwe_size = r.u64(), poly = r.u64(), base_log = r.u64(), level = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("LweBootstrapKey: " + r.err);
    if (glwe_size != (uint64_t)p->k + 1 || poly != p->N || base_log != p->pbs_base_log || level != p->pbs_level || n != want)
        return fail("LweBootstrapKey does not match the parameter set (glwe_size " + std::to_string(glwe_size) + ", N " +
                    std::to_string(poly) + ", base_log " + std::to_string(base_log) + ", level " + std::to_string(level) + ", " +
                    std::to_string(n) + " words)");
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_shortint_ciphertext(const uint64_t* ct, size_t lwe_size, const fhe_shortint_meta* meta, int safe_framing,
                                       uint8_t* out, size_t out_cap, size_t* written) {
    if (!ct || !meta || lwe_size == 0) return fail("null / empty ciphertext");
    if (meta->pbs_order > 1) return fail("pbs_order must be 0 (KeyswitchBootstrap) or 1 (BootstrapKeyswitch)");
    Writer w{out, out_cap};
    if (safe_framing) {
        w.str(kVersion);
        w.str(kShortintName);
    }
    w.vec_u64(ct, lwe_size);
    w.native_modulus_u64();
    w.u64(meta->degree);
    w.u64(meta->noise_level);
    w.u64(meta->message_modulus);
    w.u64(meta->carry_modulus);
    w.u32(meta->pbs_order);
    return finish(w, written);
}

int fhe_wire_read_shortint_ciphertext(const uint8_t* in, size_t in_len, int safe_framing, uint64_t size_limit, uint64_t* ct,
                                      size_t ct_cap, size_t* lwe_size, fhe_shortint_meta* meta, size_t* consumed) {
    if (!in || !ct || !meta) return fail("null pointer");
    Reader r{in, in_len};
    if (safe_framing) {
        const std::string version = r.str(100);          // VERSION_LENGTH_LIMIT
        if (r.err.empty() && version != kVersion)
            return fail("On deserialization, expected serialization version 0.1, got version " + version);
        const std::string name = r.str(1000);            // TYPE_NAME_LENGTH_LIMIT
        if (r.err.empty() && name != kShortintName)
            return fail("On deserialization, expected type shortint::Ciphertext, got type " + name);
    }
    const size_t body = r.pos;
    const size_t n = r.vec_u64(ct, ct_cap);
    r.native_modulus_u64();
    meta->degree = r.u64();
    meta->noise_level = r.u64();
    meta->message_modulus = r.u64();
    meta->carry_modulus = r.u64();
    meta->pbs_order = r.u32();
    if (!r.err.empty()) return fail("shortint::Ciphertext: " + r.err);
    if (size_limit && r.pos - body > size_limit) return fail("shortint::Ciphertext: serialized object exceeds the size limit");
    if (meta->pbs_order > 1) return fail("shortint::Ciphertext: unknown PBSOrder variant " + std::to_string(meta->pbs_order));
    if (n == 0) return fail("shortint::Ciphertext: empty container");
    if (lwe_size) *lwe_size = n;
    if (consumed) *consumed = r.pos;
    return 0;
}

// ---- public-key objects: compact ciphertext lists and the compact public key (csrc/compact_pk.cpp) -------------------
//   LweCompactCiphertextList<Vec<u64>>  { data, lwe_size, lwe_ciphertext_count, ciphertext_modulus }
//                                                     entities/lwe_compact_ciphertext_list.rs:18-27
//   shortint::CompactCiphertextList     { ct_list, degree, message_modulus, carry_modulus, pbs_order, noise_level }
//                                                     shortint/ciphertext/mod.rs:521-529 (pbs_order BEFORE noise_level)
//   integer::CompactCiphertextList      { ct_list: the shortint list, num_blocks_per_integer: usize }
//                                                     integer/ciphertext/mod.rs:71-78
//   LweCompactPublicKey<Vec<u64>>       { glwe_ciphertext: GlweCiphertext { data, polynomial_size, ciphertext_modulus } }
//                                                     entities/lwe_compact_public_key.rs:12-17, glwe_ciphertext.rs:286-293
static int compact_list_body_write(Writer& w, const fhe_params_t* p, const uint64_t* list, uint32_t count) {
    const size_t words = fhe_compact_list_len(p, count);
    if (!fhe_compact_pk_len(p)) return fail("compact lists need a power-of-two encryption key dimension (k*N)");
    w.vec_u64(list, words);
    w.u64((uint64_t)p->k * p->N + 1);
    w.u64(count);
    w.native_modulus_u64();
    return 0;
}

// the LweCompactCiphertextList at the reader's position; *count on success
static int compact_list_body_read(Reader& r, const char* what, const fhe_params_t* p, uint64_t* list, uint32_t max_count, uint32_t* count) {
    if (!fhe_compact_pk_len(p)) return fail("compact lists need a power-of-two encryption key dimension (k*N)");
    const size_t n = r.vec_u64(list, fhe_compact_list_len(p, max_count));
    const uint64_t lwe_size = r.u64(), cnt = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail(std::string(what) + ": " + r.err);
    if (lwe_size != (uint64_t)p->k * p->N + 1)
        return fail(std::string(what) + " does not match the parameter set (lwe_size " + std::to_string(lwe_size) + ")");
    if (cnt > max_count) return fail(std::string(what) + ": " + std::to_string(cnt) + " ciphertexts, more than the destination holds");
    // lwe_compact_ciphertext_list_size(lwe_dimension, count), entities/lwe_compact_ciphertext_list.rs:55-63
    if (n != fhe_compact_list_len(p, (uint32_t)cnt))
        return fail(std::string(what) + ": container of " + std::to_string(n) + " words does not hold " + std::to_string(cnt) + " ciphertexts");
    *count = (uint32_t)cnt;
    return 0;
}

int fhe_wire_write_compact_list(const fhe_params_t* p, const uint64_t* list, uint32_t count, uint8_t* out, size_t out_cap,
                                size_t* written) {
    if (!p || !list) return fail("null pointer");
    Writer w{out, out_cap};
    if (compact_list_body_write(w, p, list, count)) return 1;
    return finish(w, written);
}

int fhe_wire_read_compact_list(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* list, uint32_t max_count,
                               uint32_t* count, size_t* consumed) {
    if (!p || !in || !list || !count) return fail("null pointer");
    Reader r{in, in_len};
    if (compact_list_body_read(r, "LweCompactCiphertextList", p, list, max_count, count)) return 1;
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_shortint_compact_list(const fhe_params_t* p, const uint64_t* list, uint32_t count, const fhe_shortint_meta* meta,
                                         uint64_t num_blocks_per_integer, uint8_t* out, size_t out_cap, size_t* written) {
    if (!p || !list || !meta) return fail("null pointer");
    if (meta->pbs_order > 1) return fail("pbs_order must be 0 (KeyswitchBootstrap) or 1 (BootstrapKeyswitch)");
    if (meta->message_modulus != p->msg_mod || meta->carry_modulus != p->carry_mod)
        return fail("CompactCiphertextList: message / carry modulus differ from the parameter set's");
    if (num_blocks_per_integer && count % num_blocks_per_integer)
        return fail("integer CompactCiphertextList: the ciphertext count is not a multiple of num_blocks_per_integer");
    Writer w{out, out_cap};
    if (compact_list_body_write(w, p, list, count)) return 1;
    w.u64(meta->degree);
    w.u64(meta->message_modulus);
    w.u64(meta->carry_modulus);
    w.u32(meta->pbs_order);
    w.u64(meta->noise_level);
    if (num_blocks_per_integer) w.u64(num_blocks_per_integer);
    return finish(w, written);
}

int fhe_wire_read_shortint_compact_list(const fhe_params_t* p, const uint8_t* in, size_t in_len, int integer_form, uint64_t* list,
                                        uint32_t max_count, uint32_t* count, fhe_shortint_meta* meta, uint64_t* num_blocks_per_integer,
                                        size_t* consumed) {
    if (!p || !in || !list || !count || !meta || (integer_form && !num_blocks_per_integer)) return fail("null pointer");
    const char* what = integer_form ? "integer CompactCiphertextList" : "shortint CompactCiphertextList";
    Reader r{in, in_len};
    if (compact_list_body_read(r, what, p, list, max_count, count)) return 1;
    meta->degree = r.u64();
    meta->message_modulus = r.u64();
    meta->carry_modulus = r.u64();
    meta->pbs_order = r.u32();
    meta->noise_level = r.u64();
    const uint64_t blocks = integer_form ? r.u64() : 0;
    if (!r.err.empty()) return fail(std::string(what) + ": " + r.err);
    if (meta->pbs_order > 1) return fail(std::string(what) + ": unknown PBSOrder variant " + std::to_string(meta->pbs_order));
    if (meta->message_modulus != p->msg_mod || meta->carry_modulus != p->carry_mod)
        return fail(std::string(what) + " does not match the parameter set (message modulus " + std::to_string(meta->message_modulus) +
                    ", carry modulus " + std::to_string(meta->carry_modulus) + ")");
    if (integer_form && (blocks == 0 || *count % blocks))
        return fail(std::string(what) + ": " + std::to_string(*count) + " ciphertexts are not a multiple of num_blocks_per_integer " +
                    std::to_string(blocks));
    if (num_blocks_per_integer) *num_blocks_per_integer = blocks;
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_compact_public_key(const fhe_params_t* p, const uint64_t* pk, uint8_t* out, size_t out_cap, size_t* written) {
    if (!p || !pk) return fail("null pointer");
    const size_t words = fhe_compact_pk_len(p);
    if (!words) return fail("a compact public key needs a power-of-two encryption key dimension (k*N)");
    Writer w{out, out_cap};
    w.vec_u64(pk, words);
    w.u64(words / 2);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_compact_public_key(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* pk, size_t* consumed) {
    if (!p || !in || !pk) return fail("null pointer");
    const size_t want = fhe_compact_pk_len(p);
    if (!want) return fail("a compact public key needs a power-of-two encryption key dimension (k*N)");
    Reader r{in, in_len};
    const size_t n = r.vec_u64(pk, want);
    const uint64_t poly = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("LweCompactPublicKey: " + r.err);
    if (poly != want / 2 || n != want)   // GLWE size 2: mask and body polynomial
        return fail("LweCompactPublicKey does not match the parameter set (polynomial size " + std::to_string(poly) + ", " +
                    std::to_string(n) + " words)");
    if (consumed) *consumed = r.pos;
    return 0;
}

// ---- packing keyswitch objects ---------------------------------------------------------------------------------------
//   LwePackingKeyswitchKey<Vec<u64>> { data, decomp_base_log, decomp_level_count, output_glwe_size, output_polynomial_size,
//                                      ciphertext_modulus }                       entities/lwe_packing_keyswitch_key.rs
//   GlweCiphertext<Vec<u64>>         { data, polynomial_size, ciphertext_modulus }   entities/glwe_ciphertext.rs:286-293
int fhe_wire_write_packing_key(const fhe_params_t* p, const fhe_packing_params_t* pp, const uint64_t* pksk, uint8_t* out,
                               size_t out_cap, size_t* written) {
    if (!p || !pp || !pksk) return fail("null pointer");
    const size_t words = fhe_packing_key_len(p, pp);
    if (!words) return 1;                                   // reason set by the parameter check
    Writer w{out, out_cap};
    w.vec_u64(pksk, words);
    w.u64(pp->base_log);
    w.u64(pp->level);
    w.u64((uint64_t)p->k + 1);
    w.u64(p->N);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_packing_key(const fhe_params_t* p, const uint8_t* in, size_t in_len, fhe_packing_params_t* pp, uint64_t* pksk,
                              size_t pksk_cap_words, size_t* consumed) {
    if (!p || !in || !pp) return fail("null pointer");
    Reader r{in, in_len};
    const uint64_t n = r.u64();                             // the data come first: step over them to the dimensions
    if (r.err.empty() && n > (r.len - r.pos) / 8) r.err = "truncated input";
    if (!r.err.empty()) return fail("LwePackingKeyswitchKey: " + r.err);
    const size_t data_pos = r.pos;
    r.pos += (size_t)n * 8;
    const uint64_t base_log = r.u64(), level = r.u64(), glwe_size = r.u64(), poly = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("LwePackingKeyswitchKey: " + r.err);
    if (base_log > 64 || level > 64) return fail("LwePackingKeyswitchKey: decomposition out of range");
    const fhe_packing_params_t got{(uint32_t)base_log, (uint32_t)level};
    const size_t want = fhe_packing_key_len(p, &got);
    if (!want) return 1;
    if (glwe_size != (uint64_t)p->k + 1 || poly != p->N || n != want)
        return fail("LwePackingKeyswitchKey does not match the parameter set (GLWE size " + std::to_string(glwe_size) +
                    ", polynomial size " + std::to_string(poly) + ", " + std::to_string(n) + " words)");
    *pp = got;
    if (pksk) {
        if (pksk_cap_words < want) return fail("LwePackingKeyswitchKey: destination holds fewer than " + std::to_string(want) + " words");
        std::memcpy(pksk, in + data_pos, want * 8);
    }
    if (consumed) *consumed = r.pos;
    return 0;
}

// The ring packing key (csrc/ring_packing.h) in the packing key's layout: { data, decomp_base_log, decomp_level_count,
// output_glwe_size, output_polynomial_size, ciphertext_modulus }, data = [log2 N][k][level][k+1][N].  Parity unpinned.
int fhe_wire_write_ring_packing_key(const fhe_params_t* p, const fhe_packing_params_t* pp, const uint64_t* key, uint8_t* out, size_t out_cap,
                                    size_t* written) {
    if (!p || !pp || !key) return fail("null pointer");
    const size_t words = fhe_ring_packing_key_len(p, pp);
    if (!words) return 1;                                   // reason set by the parameter check
    Writer w{out, out_cap};
    w.vec_u64(key, words);
    w.u64(pp->base_log);
    w.u64(pp->level);
    w.u64((uint64_t)p->k + 1);
    w.u64(p->N);
    w.native_modulus_u64();
    return finish(w, written);
}

int fhe_wire_read_ring_packing_key(const fhe_params_t* p, const uint8_t* in, size_t in_len, fhe_packing_params_t* pp, uint64_t* key,
                                   size_t key_cap_words, size_t* consumed) {
    if (!p || !in || !pp) return fail("null pointer");
    Reader r{in, in_len};
    const uint64_t n = r.u64();                             // the data come first: step over them to the dimensions
    if (r.err.empty() && n > (r.len - r.pos) / 8) r.err = "truncated input";
    if (!r.err.empty()) return fail("RingPackingKey: " + r.err);
    const size_t data_pos = r.pos;
    r.pos += (size_t)n * 8;
    const uint64_t base_log = r.u64(), level = r.u64(), glwe_size = r.u64(), poly = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("RingPackingKey: " + r.err);
    if (base_log > 64 || level > 64) return fail("RingPackingKey: decomposition out of range");
    const fhe_packing_params_t got{(uint32_t)base_log, (uint32_t)level};
    const size_t want = fhe_ring_packing_key_len(p, &got);
    if (!want) return 1;
    if (glwe_size != (uint64_t)p->k + 1 || poly != p->N || n != want)
        return fail("RingPackingKey does not match the parameter set (GLWE size " + std::to_string(glwe_size) + ", polynomial size " +
                    std::to_string(poly) + ", " + std::to_string(n) + " words)");
    *pp = got;
    if (key) {
        if (key_cap_words < want) return fail("RingPackingKey: destination holds fewer than " + std::to_string(want) + " words");
        std::memcpy(key, in + data_pos, want * 8);
    }
    if (consumed) *consumed = r.pos;
    return 0;
}

static void glwe_body_write(Writer& w, const fhe_params_t* p, const uint64_t* glwe) {
    w.vec_u64(glwe, (size_t)(p->k + 1) * p->N);
    w.u64(p->N);
    w.native_modulus_u64();
}

static int glwe_body_read(Reader& r, const fhe_params_t* p, uint64_t* glwe) {
    const size_t want = (size_t)(p->k + 1) * p->N;
    const size_t n = r.vec_u64(glwe, want);
    const uint64_t poly = r.u64();
    r.native_modulus_u64();
    if (!r.err.empty()) return fail("GlweCiphertext: " + r.err);
    if (poly != p->N || n != want)
        return fail("GlweCiphertext does not match the parameter set (polynomial size " + std::to_string(poly) + ", " +
                    std::to_string(n) + " words)");
    return 0;
}

int fhe_wire_write_glwe_ciphertext(const fhe_params_t* p, const uint64_t* glwe, uint8_t* out, size_t out_cap, size_t* written) {
    if (!p || !glwe) return fail("null pointer");
    Writer w{out, out_cap};
    glwe_body_write(w, p, glwe);
    return finish(w, written);
}

int fhe_wire_read_glwe_ciphertext(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* glwe, size_t* consumed) {
    if (!p || !in || !glwe) return fail("null pointer");
    Reader r{in, in_len};
    if (glwe_body_read(r, p, glwe)) return 1;
    if (consumed) *consumed = r.pos;
    return 0;
}

int fhe_wire_write_glwe_list(const fhe_params_t* p, const uint64_t* glwes, uint32_t n_glwes, uint8_t* out, size_t out_cap,
                             size_t* written) {
    if (!p || (n_glwes && !glwes)) return fail("null pointer");
    Writer w{out, out_cap};
    w.u64(n_glwes);
    for (uint32_t g = 0; g < n_glwes; g++) glwe_body_write(w, p, glwes + (size_t)g * (p->k + 1) * p->N);
    return finish(w, written);
}

int fhe_wire_read_glwe_list(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* glwes, uint32_t max_glwes,
                            uint32_t* n_glwes, size_t* consumed) {
    if (!p || !in || !n_glwes || (max_glwes && !glwes)) return fail("null pointer");
    Reader r{in, in_len};
    const uint64_t n = r.u64();
    if (!r.err.empty()) return fail("GLWE list: " + r.err);
    if (n > max_glwes) return fail("GLWE list: " + std::to_string(n) + " ciphertexts, the destination holds " + std::to_string(max_glwes));
    for (uint64_t g = 0; g < n; g++)
        if (glwe_body_read(r, p, glwes + (size_t)g * (p->k + 1) * p->N)) return 1;
    *n_glwes = (uint32_t)n;
    if (consumed) *consumed = r.pos;
    return 0;
}

// The narrow list (glwe_narrow.h) is this project's own container: glwe_dimension, polynomial_size, bits and held as u64,
// then a bincode Vec<u64> of the words.
int fhe_wire_write_narrow_list(const fhe_params_t* p, const uint64_t* narrow, uint32_t held, uint32_t bits, uint8_t* out, size_t out_cap,
                               size_t* written) {
    if (!p || (held && !narrow)) return fail("null pointer");
    const size_t words = fhe::narrow_len(p->N, p->k, held, bits);
    if (held && !words) return fail("narrow list: the width must be 8 .. 32 bits and the polynomial size a power of two");
    if (const char* why = fhe::narrow_tail_check(p->N, p->k, narrow, held, bits)) return fail(why);
    Writer w{out, out_cap};
    w.u64(p->k);
    w.u64(p->N);
    w.u64(bits);
    w.u64(held);
    w.vec_u64(narrow, words);
    return finish(w, written);
}

int fhe_wire_read_narrow_list(const fhe_params_t* p, const uint8_t* in, size_t in_len, uint64_t* narrow, size_t narrow_cap_words,
                              uint32_t max_held, uint32_t* held, uint32_t* bits, size_t* consumed) {
    if (!p || !in || !held || !bits) return fail("null pointer");
    Reader r{in, in_len};
    const uint64_t k = r.u64(), N = r.u64(), b = r.u64(), h = r.u64();
    if (!r.err.empty()) return fail("narrow list: " + r.err);
    if (k != p->k || N != p->N)
        return fail("narrow list does not match the parameter set (glwe dimension " + std::to_string(k) + ", polynomial size " + std::to_string(N) + ")");
    if (b < fhe::NARROW_BITS_MIN || b > fhe::NARROW_BITS_MAX) return fail("narrow list: a width of " + std::to_string(b) + " bits, 8 .. 32 are valid");
    if (h > max_held) return fail("narrow list: " + std::to_string(h) + " blocks, the caller accepts " + std::to_string(max_held));
    const size_t want = fhe::narrow_len(p->N, p->k, (uint32_t)h, (uint32_t)b);
    if (h && !want) return fail("narrow list: unsupported polynomial size");
    const size_t at = r.pos;
    const uint64_t n = r.u64();
    if (!r.err.empty()) return fail("narrow list: " + r.err);
    if (n != want) return fail("narrow list: " + std::to_string(n) + " words, " + std::to_string(h) + " blocks at " + std::to_string(b) + " bits take " + std::to_string(want));
    if (n > (r.len - r.pos) / 8) return fail("narrow list: truncated input");
    *held = (uint32_t)h;
    *bits = (uint32_t)b;
    if (!narrow) {                                          // the header only: size the buffer with fhe_narrow_len and call again
        if (consumed) *consumed = at;
        return 0;
    }
    if (want > narrow_cap_words) return fail("narrow list: " + std::to_string(want) + " words, the destination holds " + std::to_string(narrow_cap_words));
    std::memcpy(narrow, in + r.pos, want * 8);
    r.pos += want * 8;
    if (const char* why = fhe::narrow_tail_check(p->N, p->k, narrow, *held, *bits)) return fail(why);
    if (consumed) *consumed = r.pos;
    return 0;
}

}  // extern "C"
