// cast.h -- casting keys: moving blocks from one client's key, or one parameter set, to another's.
//
// shortint::KeySwitchingKey of the reference (shortint/key_switching_key/mod.rs:17-160) is an LweKeyswitchKey from the
// source client's big LWE key to the destination's big key plus cast_rshift, the difference of the two sets' bits per
// block; a cast is the keyswitch and, where the bits differ, one lookup that shifts the value into place.  Here the same
// key is FHE_CAST_TO_BIG, and FHE_CAST_TO_SMALL is the project's own form: the key ends at the destination's SMALL key, so
// the keyswitched block is the blind rotation's input and the whole cast costs one ordinary lookup level.
//
// This header and cast.cpp are host code over standard headers only (tests/cast_main.cpp builds them alone under the
// sanitizers): the parameter checks, the default decompositions, cast_rshift, the plain keyswitch loop that pins the
// kernels, the noise of a keyswitched block.  The resident keys and the launches are fhe::CastKey's (engine.h,
// cast_dev.hip); the one kernel of its own is cast_decompose_glwe_kernel (cast_kernels.hip.h).
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/fhestr.h"

namespace fhe {

constexpr uint64_t kCastKeyMaxBytes = 1ull << 32;      // the cap the packing key has
constexpr uint32_t kCastToBigBaseLog = 1, kCastToBigLevel = 15;      // PARAM_KEYSWITCH_1_1_KS_PBS_TO_2_2_KS_PBS

// LWE dimension the key ends at: the destination's k N (TO_BIG) or n (TO_SMALL)
inline uint32_t cast_out_dim(const fhe_params_t& dst, const fhe_cast_params_t& cp) {
    return cp.target == FHE_CAST_TO_SMALL ? dst.n : dst.k * dst.N;
}
inline uint32_t cast_in_dim(const fhe_cast_params_t& cp) { return cp.src.k * cp.src.N; }
inline uint64_t cast_key_words(const fhe_params_t& dst, const fhe_cast_params_t& cp) {
    return (uint64_t)cast_in_dim(cp) * cp.level * ((uint64_t)cast_out_dim(dst, cp) + 1);
}

// Every function that can refuse returns the reason, or an empty string.
std::string cast_params_check(const fhe_params_t& dst, const fhe_cast_params_t& cp);
std::string cast_rshift(const fhe_params_t& src, const fhe_params_t& dst, int32_t* shift);
std::string cast_default_params(const fhe_params_t& src, const fhe_params_t& dst, uint32_t target, fhe_cast_params_t* cp);

// Regrouping `group` consecutive source blocks (least significant first, weights msg_src^i) into one destination block before
// the table x >> shift: *degree receives the largest lookup input, (msg_src^group - 1) << shift, *space the destination's
// msg_mod * carry_mod.  Refused unless shift > 0, msg_src^group is the destination's msg_mod and degree < space; group 1 always passes.
std::string cast_regroup_check(const fhe_params_t& src, const fhe_params_t& dst, uint32_t group, uint64_t* degree, uint64_t* space);

// lwe_keyswitch.rs:96-170 at the cast key's dimensions: count rows of in_dim + 1 words -> count rows of out_dim + 1
void cast_keyswitch_host(const fhe_params_t& dst, const fhe_cast_params_t& cp, const uint64_t* key, const uint64_t* in, uint32_t count,
                         uint64_t* out);
// fhe_cast_noise (include/fhestr.h): out[0] the next lookup's input in the destination's nominal units, out[1] its
// PBS-input budget, out[2] the keyswitched block's torus variance
void cast_noise(const fhe_params_t& dst, const fhe_cast_params_t& cp, double v_in, double out[3]);
// the same for a sum of keyswitched blocks whose squared weights add up to `weight` (regrouping, CastKey::set_group)
void cast_noise_weighted(const fhe_params_t& dst, const fhe_cast_params_t& cp, double v_in, double weight, double out[3]);
// The table that follows the keyswitch: x -> x >> shift over the destination's message-and-carry space (shift >= 0; the
// identity at 0), `table` of dst.msg_mod * dst.carry_mod entries
void cast_shift_table(const fhe_params_t& dst, int32_t shift, uint64_t* table);

}  // namespace fhe
