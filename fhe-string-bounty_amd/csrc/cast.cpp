// cast.cpp -- the host side of casting keys (cast.h): parameter checks and defaults, cast_rshift, the keyswitch in plain
// loops that pins the kernels of cast_dev.hip, and the noise of a keyswitched block.  Standard headers only, no engine, no
// device: tests/cast_main.cpp links this file alone.  The C entry points of these are in client.cpp, next to the key
// generation they share with the clients' own keyswitch keys.
#include "cast.h"

#include <cstring>
#include <vector>

#include "noise_model.h"

namespace fhe {

static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }
static int32_t ilog2(uint64_t x) {
    int32_t b = 0;
    while (x >>= 1) b++;
    return b;
}

std::string cast_rshift(const fhe_params_t& src, const fhe_params_t& dst, int32_t* shift) {
    const uint64_t m1 = (uint64_t)src.msg_mod * src.carry_mod, m2 = (uint64_t)dst.msg_mod * dst.carry_mod;
    if (!pow2(m1) || !pow2(m2))      // mod.rs:66-69
        return "casting key: the message-and-carry moduli must be powers of two (source " + std::to_string(m1) + ", destination " + std::to_string(m2) + ")";
    *shift = ilog2(m2) - ilog2(m1);
    return {};
}

std::string cast_params_check(const fhe_params_t& dst, const fhe_cast_params_t& cp) {
    if (cp.target != FHE_CAST_TO_BIG && cp.target != FHE_CAST_TO_SMALL) return "casting key: the target must be FHE_CAST_TO_BIG or FHE_CAST_TO_SMALL";
    if (cp.src.k < 1 || cp.src.N < 1 || dst.k < 1 || dst.N < 1 || dst.n < 1) return "casting key: empty source or destination dimensions";
    if ((uint64_t)cp.src.k * cp.src.N > (1u << 20)) return "casting key: the source key has more than 2^20 bits";
    if (cp.level < 1 || cp.level > 16)
        return "casting key: " + std::to_string(cp.level) + " levels, the matrix-core keyswitch takes 1 .. 16";
    if (cp.base_log < 1 || cp.base_log > 7) return "casting key: base_log " + std::to_string(cp.base_log) + ", the keyswitch digits take 1 .. 7";
    if (cp.base_log * cp.level > 63) return "casting key: base_log * level must be at most 63";
    int32_t shift;
    const std::string why = cast_rshift(cp.src, dst, &shift);
    if (!why.empty()) return why;
    const uint64_t bytes = cast_key_words(dst, cp) * 8;
    if (bytes > kCastKeyMaxBytes)
        return "casting key: the key would hold " + std::to_string(bytes) + " bytes (limit 4 GiB)" +
               (cp.target == FHE_CAST_TO_BIG ? "; FHE_CAST_TO_SMALL ends at the destination's small key" : "");
    return {};
}

std::string cast_default_params(const fhe_params_t& src, const fhe_params_t& dst, uint32_t target, fhe_cast_params_t* cp) {
    cp->src = src;
    cp->target = target;
    cp->base_log = target == FHE_CAST_TO_SMALL ? dst.ks_base_log : kCastToBigBaseLog;
    cp->level = target == FHE_CAST_TO_SMALL ? dst.ks_level : kCastToBigLevel;
    return cast_params_check(dst, *cp);
}

std::string cast_regroup_check(const fhe_params_t& src, const fhe_params_t& dst, uint32_t group, uint64_t* degree, uint64_t* space) {
    int32_t shift = 0;
    const std::string why = cast_rshift(src, dst, &shift);
    if (!why.empty()) return why;
    *space = (uint64_t)dst.msg_mod * dst.carry_mod;
    if (group < 1 || group > 32) return "cast regrouping: 1 .. 32 source blocks per destination block";
    uint64_t top = 1;
    for (uint32_t i = 0; i < group && top <= (1ull << 32); i++) top *= src.msg_mod;
    *degree = shift >= 0 ? ((top - 1) << shift) : ((top - 1) >> -shift);
    if (group == 1) return {};
    if (shift <= 0) return "cast regrouping: only a cast to more bits per block regroups (cast_rshift " + std::to_string(shift) + ")";
    if (*degree >= *space)
        return "cast regrouping: " + std::to_string(group) + " source blocks give a lookup input of up to " + std::to_string(*degree) +
               ", the destination's message-and-carry space ends at " + std::to_string(*space - 1);
    if (top != dst.msg_mod) return "cast regrouping: " + std::to_string(group) + " source blocks do not fill one destination block";
    return {};
}

// signed digits of the closest representable value, level L first (decomposer.rs:98-152, iter.rs:101-127)
static inline void cast_decompose(uint64_t x, uint32_t bl, uint32_t L, int64_t* digits) {
    const uint32_t rep = bl * L;
    const uint64_t mask = (1ull << bl) - 1;
    uint64_t state = (((x >> (63 - rep)) + 1) >> 1) & ((1ull << rep) - 1);
    for (uint32_t lv = 0; lv < L; lv++) {
        uint64_t res = state & mask;
        state >>= bl;
        uint64_t carry = (((res - 1ull) | state) & res) >> (bl - 1);
        state += carry;
        digits[lv] = (int64_t)res - (int64_t)(carry << bl);
    }
}

void cast_keyswitch_host(const fhe_params_t& dst, const fhe_cast_params_t& cp, const uint64_t* key, const uint64_t* in, uint32_t count,
                         uint64_t* out) {
    const size_t in_dim = cast_in_dim(cp), out_size = (size_t)cast_out_dim(dst, cp) + 1;
    int64_t digits[16];
    for (uint32_t b = 0; b < count; b++) {
        const uint64_t* ct = in + (size_t)b * (in_dim + 1);
        uint64_t* o = out + (size_t)b * out_size;
        std::memset(o, 0, out_size * 8);
        o[out_size - 1] = ct[in_dim];
        for (size_t i = 0; i < in_dim; i++) {
            cast_decompose(ct[i], cp.base_log, cp.level, digits);
            for (uint32_t lv = 0; lv < cp.level; lv++) {
                if (!digits[lv]) continue;
                const uint64_t d = (uint64_t)digits[lv], *row = key + (i * cp.level + lv) * out_size;
                for (size_t c = 0; c < out_size; c++) o[c] -= d * row[c];
            }
        }
    }
}

// NoiseModel::v_ks with the cast key's in_dim, pair and noise (the destination's lwe_std for both targets: TO_BIG as
// new_key_switching_key chooses it, TO_SMALL because the rows are encryptions under the small key)
void cast_noise(const fhe_params_t& dst, const fhe_cast_params_t& cp, double v_in, double out[3]) { cast_noise_weighted(dst, cp, v_in, 1.0, out); }

void cast_noise_weighted(const fhe_params_t& dst, const fhe_cast_params_t& cp, double v_in, double weight, double out[3]) {
    const double in_dim = cast_in_dim(cp), B = ldexp(1.0, (int)cp.base_log);
    const double v_cast = in_dim * cp.level * (B * B + 2) / 12.0 * dst.lwe_std * dst.lwe_std + in_dim / 2.0 / (12.0 * pow(B, 2.0 * cp.level));
    const NoiseModel ms = noise_model(cp.src), md = noise_model(dst);
    out[2] = weight * (v_in * ms.v_pbs + v_cast);
    out[0] = cp.target == FHE_CAST_TO_SMALL ? (out[2] > md.v_ks ? (out[2] - md.v_ks) / md.v_pbs : 0.0) : out[2] / md.v_pbs;
    out[1] = default_noise_budget(dst);
}

void cast_shift_table(const fhe_params_t& dst, int32_t shift, uint64_t* table) {
    const uint32_t M = dst.msg_mod * dst.carry_mod;
    for (uint32_t x = 0; x < M; x++) table[x] = shift > 0 ? x >> shift : x;
}

}  // namespace fhe
