"""Everything that talks to ctypes: where libfhestr.so is, the structures of include/fhestr.h, ONE table of every entry
point's signature -- the only place that knows the C ABI -- and the few marshalling idioms the binding modules share.
lib() applies the whole table once, at load; EXPORTS is read off it."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FHESTR_LIB: load another build of the same library (kernel A/B experiments, scripts/ab_bench.sh)
LIB_PATH = os.environ.get("FHESTR_LIB") or os.path.join(os.path.dirname(_HERE), "libfhestr.so")


class FheError(RuntimeError):
    pass


class _Params(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("k", C.c_uint32), ("N", C.c_uint32),
        ("pbs_base_log", C.c_uint32), ("pbs_level", C.c_uint32),
        ("ks_base_log", C.c_uint32), ("ks_level", C.c_uint32),
        ("msg_mod", C.c_uint32), ("carry_mod", C.c_uint32),
        ("lwe_std", C.c_double), ("glwe_std", C.c_double),
        ("grouping_factor", C.c_uint32),
    ]


class _PackingParams(C.Structure):
    _fields_ = [("base_log", C.c_uint32), ("level", C.c_uint32)]


class _CastParams(C.Structure):
    _fields_ = [("src", _Params), ("base_log", C.c_uint32), ("level", C.c_uint32), ("target", C.c_uint32)]


class _Meta(C.Structure):
    _fields_ = [("degree", C.c_uint64), ("noise_level", C.c_uint64), ("message_modulus", C.c_uint64),
                ("carry_modulus", C.c_uint64), ("pbs_order", C.c_uint32)]


def _signatures():
    """The signature table, name -> (restype, argtypes), in the order of the sections of include/fhestr.h: (what the
    header declares, what the library exports beside it).  The short type names live in here alone."""
    vp, cs, sz, i32, u32, i64, u64, f64 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_double
    vpp, szp, i32p, u32p, u64p, f32p, f64p = (C.POINTER(t) for t in (vp, sz, C.c_int32, u32, u64, C.c_float, f64))
    PP, KP, CP, MP = (C.POINTER(t) for t in (_Params, _PackingParams, _CastParams, _Meta))
    binary = ("eq", "ne", "starts_with", "ends_with", "contains", "find", "rfind", "eq_ignore_case", "lt", "le", "gt", "ge", "concat")

    header = {
        "fhe_last_error": (cs, ()),
        "fhe_kernel_revision": (cs, ()),
        # ---- engine + keys ----
        "fhe_engine_create": (i32, (PP, i32, vpp)),
        "fhe_engine_destroy": (i32, (vp,)),
        "fhe_engine_params": (i32, (vp, PP)),
        "fhe_engine_load_keys": (i32, (vp, vp, vp)),
        "fhe_engine_generate_keys": (i32, (vp, vp, vp, vp, vp, vp)),
        "fhe_engine_stream": (vp, (vp,)),
        "fhe_engine_set_stream": (i32, (vp, vp)),
        "fhe_engine_reset_stream": (i32, (vp,)),
        "fhe_engine_synchronize": (i32, (vp,)),
        "fhe_engine_set_variant": (i32, (vp, i32)),
        "fhe_engine_set_pipeline": (i32, (vp, i32)),
        "fhe_engine_pipeline_input_event": (i32, (vp, vp)),
        "fhe_engine_set_multibit_combine_max": (i32, (vp, u32)),
        "fhe_engine_set_cluster_mode": (i32, (vp, i32, u32)),
        "fhe_engine_set_keep_busy": (i32, (vp, i32)),
        "fhe_engine_cluster_info": (i32, (vp, u32p)),
        "fhe_engine_keyswitch_info": (i32, (vp, u32p)),
        "fhe_engine_cluster_fallbacks": (i32, (vp, u32p)),
        # ---- lookup tables ----
        "fhe_lut_generate": (i32, (vp, vp, u32p, u64p)),
        "fhe_lut_upload": (i32, (vp, vp, u32p)),
        "fhe_lut_download": (i32, (vp, u32, vp)),
        "fhe_lut_count": (i32, (vp, u32p)),
        # ---- the hot path ----
        "fhe_keyswitch_batch": (i32, (vp, vp, vp, u32)),
        "fhe_pbs_batch": (i32, (vp, vp, vp, vp, u32)),
        "fhe_ks_pbs_batch": (i32, (vp, vp, vp, vp, u32)),
        "fhe_pbs_ks_batch": (i32, (vp, vp, vp, vp, u32)),
        "fhe_ks_pbs_batch_dev": (i32, (vp, vp, vp, vp, u32)),
        "fhe_lwe_lincomb_batch": (i32, (vp, vp, u32, vp, vp, vp, vp, vp, u32)),
        "fhe_last_kernel_ms": (i32, (vp, f32p)),
        "fhe_kernel_times": (i32, (vp, f64p, u32p, i32)),
        # ---- plans: levelised shortint circuits ----
        "fhe_plan_create": (i32, (vp, vpp)),
        "fhe_plan_create_offline": (i32, (PP, vpp)),
        "fhe_plan_destroy": (i32, (vp,)),
        "fhe_plan_input": (i32, (vp, u64, u32p)),
        "fhe_plan_lut": (i32, (vp, vp, u32p)),
        "fhe_plan_lin": (i32, (vp, vp, vp, u32, i64, u32p)),
        "fhe_plan_pbs": (i32, (vp, u32, u32, u32p)),
        "fhe_plan_pbs_signed": (i32, (vp, u32, u32, u32p)),
        "fhe_plan_pbs_full_box": (i32, (vp, u32, i32, u32p)),
        "fhe_plan_set_noise_budget": (i32, (vp, f64)),
        "fhe_plan_set_owner_hint": (i32, (vp, i32)),
        "fhe_plan_output": (i32, (vp, u32)),
        "fhe_plan_finalize": (i32, (vp, u32)),
        "fhe_plan_info": (i32, (vp, u32p)),
        "fhe_plan_noise_info": (i32, (vp, f64p)),
        "fhe_noise_model": (i32, (PP, f64p)),
        "fhe_host_alloc": (i32, (sz, vpp)),
        "fhe_host_free": (i32, (vp,)),
        "fhe_noise_model_is_calibrated": (i32, (PP,)),
        "fhe_params_supported": (i32, (PP,)),
        "fhe_plan_level_info": (i32, (vp, u32, u32p)),
        "fhe_plan_level_rank_info": (i32, (vp, u32, u32, u32p)),
        "fhe_plan_export_level": (i32, (vp, u32, vp, vp, vp, vp, vp)),
        "fhe_plan_lut_count": (i32, (vp, u32p)),
        "fhe_plan_export_lut": (i32, (vp, u32, vp)),
        "fhe_plan_run": (i32, (vp, vp, vp)),
        "fhe_plan_run_batch": (i32, (vp, u32, vp, vp)),
        "fhe_plan_run_batch_dev": (i32, (vp, u32, vp, vp)),
        "fhe_plan_run_level_rank_dev": (i32, (vp, vp, u32, u32)),
        "fhe_plan_gather_outputs_dev": (i32, (vp, vp, vp)),
        # ---- radix-integer operations ----
        "fhe_int_plan_create": (i32, (vp, cs, u32, u64, u32, vpp)),
        "fhe_int_plan_create_offline": (i32, (PP, cs, u32, u64, u32, vpp)),
        # ---- FheString operations ----
        "fhe_str_plan_create": (i32, (vp, cs, u32, u32, vp, u32, u32, vpp)),
        "fhe_str_plan_create_offline": (i32, (PP, cs, u32, u32, vp, u32, u32, vpp)),
        **{f"fhe_str_{n}{s}": (i32, (vp, vp, u32, vp, u32, vp)) for n in binary for s in ("", "_clear")},   # FHE_STR_BINARY_DECL
        "fhe_str_matches_clear": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_regex_check": (i32, (vp, u32, u32p, u32p)),
        "fhe_str_repeat_clear": (i32, (vp, vp, u32, u32, vp)),
        "fhe_str_trim_start": (i32, (vp, vp, u32, vp)),
        "fhe_str_trim_end": (i32, (vp, vp, u32, vp)),
        "fhe_str_strip": (i32, (vp, vp, u32, vp)),
        "fhe_str_replace_general": (i32, (vp, vp, u32, vp, u32, vp, u32, u32, vp)),
        "fhe_str_replace_clear_general": (i32, (vp, vp, u32, vp, u32, vp, u32, u32, vp)),
        "fhe_str_replace": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_replace_clear": (i32, (vp, vp, u32, vp, vp, u32, vp)),
        "fhe_str_replacen": (i32, (vp, vp, u32, vp, u32, vp, u32, u32, u32, vp)),
        "fhe_str_replacen_clear": (i32, (vp, vp, u32, vp, u32, vp, u32, u32, u32, vp)),
        "fhe_str_split": (i32, (vp, cs, vp, u32, vp, u32, vp, u32, u32, u32, vp, u32p)),
        # ---- encrypted counts ----
        "fhe_str_repeat": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_replacen_encn": (i32, (vp, vp, u32, vp, u32, vp, u32, vp, u32, u32, vp)),
        "fhe_str_replacen_encn_clear": (i32, (vp, vp, u32, vp, u32, vp, u32, vp, u32, u32, vp)),
        "fhe_str_splitn_encn": (i32, (vp, cs, vp, u32, vp, u32, vp, u32, vp, u32, u32, vp, u32p)),
        # ---- slicing at a position ----
        "fhe_str_slice": (i32, (vp, cs, vp, u32, vp, u32, vp, u32, vp, u32, u32, vp, u32p)),
        # ---- combining results: bit logic, select, arithmetic on counts ----
        "fhe_str_combine": (i32, (vp, cs, vp, vp, u32, vp, u32, vp, u32p)),
        "fhe_str_op": (i32, (vp, cs, vp, vp, u32, vp, vp, u32, vp, u32p)),
        "fhe_str_op_many": (i32, (vp, cs, vp, u32, u32, vp, u32, vp, u32, vp, u32p)),
        "fhe_str_len": (i32, (vp, vp, u32, vp)),
        "fhe_str_is_empty": (i32, (vp, vp, u32, vp)),
        "fhe_str_strip_prefix_clear": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_strip_suffix_clear": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_strip_prefix": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_strip_suffix": (i32, (vp, vp, u32, vp, u32, vp)),
        "fhe_str_to_upper": (i32, (vp, vp, u32, vp)),
        "fhe_str_to_lower": (i32, (vp, vp, u32, vp)),
        # ---- string programs ----
        "fhe_str_program_create": (i32, (vp, vpp)),
        "fhe_str_program_create_offline": (i32, (PP, vpp)),
        "fhe_str_program_destroy": (i32, (vp,)),
        "fhe_str_program_set_dedupe": (i32, (vp, i32)),
        "fhe_str_program_input_string": (i32, (vp, u32, u32p)),
        "fhe_str_program_input_count": (i32, (vp, u32, u32p)),
        "fhe_str_program_input_bit": (i32, (vp, u32p)),
        "fhe_str_program_op": (i32, (vp, cs, vp, u32, vp, u32, vp, u32, u32p)),
        "fhe_str_program_value_info": (i32, (vp, u32, u32p)),
        "fhe_str_program_output": (i32, (vp, u32)),
        "fhe_str_program_finish": (i32, (vp, u32, vpp)),
        # ---- client side (CPU): keys, encryption, decryption ----
        "fhe_random_seed": (i32, (vp,)),
        "fhe_chacha20_block": (i32, (vp, u64, u64, vp)),
        "fhe_params_ksk_len": (sz, (PP,)),
        "fhe_params_bsk_len": (sz, (PP,)),
        "fhe_client_key_create": (i32, (PP, vp, vpp)),
        "fhe_client_key_destroy": (i32, (vp,)),
        "fhe_client_encrypt": (i32, (vp, vp, u32, vp)),
        "fhe_client_decrypt": (i32, (vp, vp, u32, vp)),
        "fhe_client_gen_server_keys": (i32, (vp, vp, vp, i32)),
        "fhe_client_secret_keys": (i32, (vp, vp, vp)),
        # ---- public-key clients: compact public keys and compact ciphertext lists ----
        "fhe_compact_pk_len": (sz, (PP,)),
        "fhe_compact_list_len": (sz, (PP, u32)),
        "fhe_client_gen_compact_public_key": (i32, (vp, vp, vp)),
        "fhe_compact_pk_encrypt": (i32, (PP, vp, vp, vp, u32, vp, i32)),
        "fhe_compact_expand_host": (i32, (u32, vp, u32, vp)),
        "fhe_engine_expand_compact_list": (i32, (vp, vp, u32, vp, vp)),
        "fhe_engine_expand_compact_list_dev": (i32, (vp, vp, u32, vp)),
        "fhe_compact_conv": (i32, (vp, vp, u32, vp, i32)),
        # ---- packing keyswitch: results go back as GLWE ciphertexts ----
        "fhe_packing_default_params": (i32, (PP, KP)),
        "fhe_packing_key_len": (sz, (PP, KP)),
        "fhe_packed_glwe_len": (sz, (PP, u32)),
        "fhe_client_gen_packing_key": (i32, (vp, KP, vp, vp, i32)),
        "fhe_client_decrypt_packed": (i32, (vp, vp, u32, vp)),
        "fhe_packing_keyswitch_host": (i32, (PP, KP, vp, vp, u32, vp)),
        "fhe_engine_load_packing_key": (i32, (vp, KP, vp)),
        "fhe_engine_pack_lwes": (i32, (vp, vp, u32, vp)),
        "fhe_engine_pack_lwes_dev": (i32, (vp, vp, u32, vp)),
        "fhe_engine_packing_info": (i32, (vp, u32p)),
        # ---- ring packing: the same packed GLWEs through log2(N) automorphism keys ----
        "fhe_ring_packing_default_params": (i32, (PP, KP)),
        "fhe_ring_packing_key_len": (sz, (PP, KP)),
        "fhe_ring_packing_noise": (i32, (PP, KP, f64p)),
        "fhe_ring_narrow_noise": (i32, (PP, KP, u32, f64p)),
        "fhe_ring_pack_keyswitches": (u64, (PP, u32)),
        "fhe_client_gen_ring_packing_key": (i32, (vp, KP, vp, vp, i32)),
        "fhe_ring_pack_host": (i32, (PP, KP, vp, vp, u32, vp)),
        "fhe_ring_ntt_host": (i32, (u32, i32, vp, u32)),
        "fhe_ring_product_host": (i32, (u32, u32, vp, vp, vp)),
        "fhe_engine_load_ring_packing_key": (i32, (vp, KP, vp)),
        "fhe_engine_ring_pack_lwes": (i32, (vp, vp, u32, vp)),
        "fhe_engine_ring_pack_lwes_dev": (i32, (vp, vp, u32, vp)),
        "fhe_engine_ring_pack_info": (i32, (vp, u64p)),
        "fhe_engine_ring_ntt": (i32, (vp, u32, i32, vp, u32)),
        # ---- packed GLWE ciphertexts as inputs: sample extraction at any coefficient ----
        "fhe_glwe_sample_extract_host": (i32, (PP, vp, u32, u32, vp)),
        "fhe_packing_unpack_noise": (i32, (PP, KP, f64p)),
        "fhe_engine_unpack_glwes": (i32, (vp, vp, u32, u32, i32, vp)),
        "fhe_engine_unpack_glwes_dev": (i32, (vp, vp, u32, u32, i32, vp)),
        "fhe_engine_unpack_info": (i32, (vp, u32p)),
        # ---- narrow packed results: b-bit coefficients ----
        "fhe_narrow_noise": (i32, (PP, KP, u32, f64p)),
        "fhe_narrow_default_bits": (i32, (PP, KP, i32, u32p)),
        "fhe_narrow_len": (sz, (PP, u32, u32)),
        "fhe_glwe_narrow_host": (i32, (PP, vp, u32, u32, vp)),
        "fhe_glwe_widen_host": (i32, (PP, vp, u32, u32, vp)),
        "fhe_narrow_sample_extract_host": (i32, (PP, vp, u32, u32, u32, u32, vp)),
        "fhe_client_decrypt_narrow": (i32, (vp, vp, u32, u32, vp)),
        "fhe_engine_narrow_glwes": (i32, (vp, vp, u32, u32, vp)),
        "fhe_engine_narrow_glwes_dev": (i32, (vp, vp, u32, u32, vp)),
        "fhe_engine_widen_narrow_dev": (i32, (vp, vp, u32, u32, vp)),
        "fhe_engine_unpack_narrow": (i32, (vp, vp, u32, u32, u32, u32, i32, vp)),
        "fhe_engine_unpack_narrow_dev": (i32, (vp, vp, u32, u32, u32, u32, i32, vp)),
        "fhe_engine_narrow_info": (i32, (vp, u32p)),
        # ---- transciphering ----
        "fhe_stream_cipher_info": (i32, (u32, u32p)),
        "fhe_stream_cipher_keystream": (i32, (u32, vp, vp, u64, vp, sz)),
        "fhe_transcipher_supported": (i32, (PP, u32)),
        "fhe_transcipher_table": (i32, (PP, u32, vp, u32p)),
        "fhe_transcipher_ring_len": (sz, (PP, u32)),
        "fhe_transcipher_init_host": (i32, (PP, u32, u32, vp, vp, vp)),
        "fhe_transcipher_gather_host": (i32, (PP, u32, u32, i32, u32, vp, vp, vp, vp, u32, u32, vp, vp)),
        "fhe_transcipher_apply_host": (i32, (PP, u32, u32, i32, vp, u32, u32, vp)),
        "fhe_engine_transcipher_init": (i32, (vp, u32, u32, vp, vp, vp)),
        "fhe_engine_transcipher_gather": (i32, (vp, u32, u32, i32, u32, vp, vp, vp, vp, u32, u32, vp, vp)),
        "fhe_engine_transcipher_apply": (i32, (vp, u32, u32, i32, vp, u32, u32, vp)),
        "fhe_transcipher_create": (i32, (vp, u32, vp, u32, vpp)),
        "fhe_transcipher_destroy": (i32, (vp,)),
        "fhe_transcipher_begin": (i32, (vp, vp, u32)),
        "fhe_transcipher_next": (i32, (vp, vp, u32, i32, vp, vp)),
        "fhe_transcipher_info": (i32, (vp, u32p)),
        "fhe_transcipher_timing": (i32, (vp, i32, f64p, u32p)),
        # ---- casting keys ----
        "fhe_cast_default_params": (i32, (PP, PP, u32, CP)),
        "fhe_cast_key_len": (sz, (PP, CP)),
        "fhe_cast_rshift": (i32, (PP, PP, i32p)),
        "fhe_client_gen_cast_key": (i32, (vp, vp, CP, vp, vp)),
        "fhe_cast_host": (i32, (PP, CP, vp, vp, u32, vp)),
        "fhe_cast_noise": (i32, (PP, CP, f64, f64p)),
        "fhe_cast_key_create": (i32, (vp, CP, vp, vpp)),
        "fhe_cast_key_destroy": (i32, (vp,)),
        "fhe_cast_key_info": (i32, (vp, u32p)),
        "fhe_cast_key_set_fused": (i32, (vp, i32)),
        "fhe_cast_key_set_group": (i32, (vp, u32)),
        "fhe_cast_regroup_check": (i32, (PP, PP, u32, u64p, u64p)),
        "fhe_cast_key_set_input_noise": (i32, (vp, f64)),
        "fhe_cast_lwes": (i32, (vp, vp, u32, i32, vp)),
        "fhe_cast_lwes_dev": (i32, (vp, vp, u32, i32, vp)),
        "fhe_cast_packed": (i32, (vp, vp, u32, u32, i32, vp)),
        "fhe_cast_packed_dev": (i32, (vp, vp, u32, u32, i32, vp)),
        "fhe_cast_narrow": (i32, (vp, vp, u32, u32, u32, u32, i32, vp)),
        "fhe_cast_narrow_dev": (i32, (vp, vp, u32, u32, u32, u32, i32, vp)),
        "fhe_cast_debug_digits": (i32, (vp, vp, u32, u32, i32, vp, szp)),
        # ---- tfhe-rs wire format ----
        "fhe_wire_write_lwe_ciphertext": (i32, (vp, sz, vp, sz, szp)),
        "fhe_wire_read_lwe_ciphertext": (i32, (vp, sz, vp, sz, szp, szp)),
        "fhe_wire_write_keyswitch_key": (i32, (PP, vp, vp, sz, szp)),
        "fhe_wire_read_keyswitch_key": (i32, (PP, vp, sz, vp, szp)),
        "fhe_wire_write_bootstrap_key": (i32, (PP, vp, vp, sz, szp)),
        "fhe_wire_read_bootstrap_key": (i32, (PP, vp, sz, vp, szp)),
        "fhe_wire_write_shortint_ciphertext": (i32, (vp, sz, MP, i32, vp, sz, szp)),
        "fhe_wire_read_shortint_ciphertext": (i32, (vp, sz, i32, u64, vp, sz, szp, MP, szp)),
        # ---- seeded ("compressed") server keys, and the wire objects that came after them ----
        "fhe_engine_load_seeded_keys": (i32, (vp, vp, vp, vp, vp, vp, vp)),
        "fhe_engine_expand_seeded_lwe": (i32, (vp, vp, vp, u32, vp, vp)),
        "fhe_seeded_decompress_lwe_batch": (i32, (u32, vp, vp, u32, vp)),
        "fhe_wire_write_compressed_ciphertext": (i32, (u64, sz, vp, MP, vp, sz, szp)),
        "fhe_wire_read_compressed_ciphertext": (i32, (vp, sz, u64p, szp, vp, MP, szp)),
        "fhe_wire_write_radix_ciphertext": (i32, (vp, sz, vp, sz, vp, sz, szp)),
        "fhe_wire_read_radix_ciphertext": (i32, (vp, sz, vp, sz, sz, vp, szp, szp)),
        "fhe_wire_write_compressed_radix_ciphertext": (i32, (vp, vp, sz, vp, sz, vp, sz, szp)),
        "fhe_wire_read_compressed_radix_ciphertext": (i32, (vp, sz, vp, vp, szp, sz, vp, szp, szp)),
        "fhe_aes128_encrypt_block": (i32, (vp, vp, vp)),
        "fhe_seeded_mask_words": (i32, (vp, vp, sz)),
        "fhe_seeded_decompress_keyswitch_key": (i32, (PP, vp, vp, vp)),
        "fhe_seeded_decompress_bootstrap_key": (i32, (PP, vp, vp, vp)),
        "fhe_seeded_split_keyswitch_key": (i32, (PP, vp, vp)),
        "fhe_seeded_split_bootstrap_key": (i32, (PP, vp, vp)),
        "fhe_wire_write_seeded_keyswitch_key": (i32, (PP, vp, vp, vp, sz, szp)),
        "fhe_wire_read_seeded_keyswitch_key": (i32, (PP, vp, sz, vp, vp, szp)),
        "fhe_wire_write_seeded_bootstrap_key": (i32, (PP, vp, vp, vp, sz, szp)),
        "fhe_wire_read_seeded_bootstrap_key": (i32, (PP, vp, sz, vp, vp, szp)),
        "fhe_wire_write_compressed_server_key": (i32, (PP, vp, vp, vp, vp, u64, u32, vp, sz, szp)),
        "fhe_wire_read_compressed_server_key": (i32, (PP, vp, sz, vp, vp, vp, vp, u64p, u32p, szp)),
        "fhe_wire_write_multi_bit_bootstrap_key": (i32, (PP, vp, vp, sz, szp)),
        "fhe_wire_read_multi_bit_bootstrap_key": (i32, (PP, vp, sz, vp, szp)),
        "fhe_wire_write_compact_list": (i32, (PP, vp, u32, vp, sz, szp)),
        "fhe_wire_read_compact_list": (i32, (PP, vp, sz, vp, u32, u32p, szp)),
        "fhe_wire_write_shortint_compact_list": (i32, (PP, vp, u32, MP, u64, vp, sz, szp)),
        "fhe_wire_read_shortint_compact_list": (i32, (PP, vp, sz, i32, vp, u32, u32p, MP, u64p, szp)),
        "fhe_wire_write_compact_public_key": (i32, (PP, vp, vp, sz, szp)),
        "fhe_wire_read_compact_public_key": (i32, (PP, vp, sz, vp, szp)),
        "fhe_wire_write_packing_key": (i32, (PP, KP, vp, vp, sz, szp)),
        "fhe_wire_read_packing_key": (i32, (PP, vp, sz, KP, vp, sz, szp)),
        "fhe_wire_write_ring_packing_key": (i32, (PP, KP, vp, vp, sz, szp)),
        "fhe_wire_read_ring_packing_key": (i32, (PP, vp, sz, KP, vp, sz, szp)),
        "fhe_wire_write_glwe_ciphertext": (i32, (PP, vp, vp, sz, szp)),
        "fhe_wire_read_glwe_ciphertext": (i32, (PP, vp, sz, vp, szp)),
        "fhe_wire_write_glwe_list": (i32, (PP, vp, u32, vp, sz, szp)),
        "fhe_wire_read_glwe_list": (i32, (PP, vp, sz, vp, u32, u32p, szp)),
        "fhe_wire_write_narrow_list": (i32, (PP, vp, u32, u32, vp, sz, szp)),
        "fhe_wire_read_narrow_list": (i32, (PP, vp, sz, vp, sz, u32, u32p, u32p, szp)),
    }

    # The library exports these for the tests; include/fhestr.h does not declare them, so they are no part of EXPORTS.
    not_in_header = {
        "fhe_debug_det_log": (i32, (vp, sz, vp)),
        "fhe_debug_noise_samples": (i32, (vp, u64, f64, sz, vp)),
        "fhe_debug_round_torus": (i32, (vp, sz, vp, vp)),
    }
    return header, not_in_header


_HEADER, _NOT_IN_HEADER = _signatures()
EXPORTS = list(_HEADER)

_lib = None


def lib() -> C.CDLL:
    """Load libfhestr.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FheError(f"{LIB_PATH} is missing: run `make -C fhe-string-bounty_amd` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64: two HIP runtimes in
    # one process do not see the same device (the second one finds no GPU) and cannot share streams.
    # Importing torch first makes its copy the process-wide one; libfhestr.so (NEEDED libamdhip64.so.7)
    # then binds to it, so torch streams / tensors and the engine live in a single runtime.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**_HEADER, **_NOT_IN_HEADER}.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = L
    return L


# ---- marshalling shared by the binding modules ----
def _last_error() -> str:
    return lib().fhe_last_error().decode()


def _check(rc: int):
    if rc != 0:
        raise FheError(_last_error() or "fhestr call failed")


def _nonzero(n: int) -> int:
    """The answer of a size query (fhe_*_len): 0 says the library refused the parameters and left the reason."""
    if not n:
        raise FheError(_last_error())
    return int(n)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(a: "np.ndarray | None"):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _in(data: bytes):
    """Clear bytes as an argument: never a zero-length buffer, the length travels beside it."""
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")


def _clear(clear: "bytes | None"):
    """The clear bytes of a call as its two arguments (buffer, length); (NULL, 0) for a call that takes none."""
    return (None, 0) if clear is None else (_in(clear), len(clear))


def _record(ctype, n: int, call, *args) -> list:
    """The n values an *_info style entry point writes behind its last argument (Python ints, or floats)."""
    a = (ctype * n)()
    _check(call(*args, a))
    return list(a)


def seed_bytes(seed) -> bytes:
    """256-bit seed (ChaCha20 key) as 32 bytes.  Tests pass small integers (little endian, zero extended);
    production code passes random_seed()."""
    if isinstance(seed, (bytes, bytearray)):
        if len(seed) != 32:
            raise FheError("a seed is 32 bytes")
        return bytes(seed)
    return int(seed).to_bytes(32, "little")


class _Handle:
    """An object of the library behind self._h.  close() destroys it once, through the entry point named by `_destroy`;
    a class whose objects the engine owns (`_engine_owned`: gone with the engine at the latest) only forgets the handle
    once its engine has been closed.  __del__ closes what was left open."""
    _destroy: str
    _engine_owned = False

    def close(self):
        if self._h and not (self._engine_owned and not self.engine._h):
            getattr(lib(), self._destroy)(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
