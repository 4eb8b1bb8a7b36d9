"""fhestr -- ctypes binding of libfhestr.so (the C ABI in include/fhestr.h).

This is the thin host-side mirror used by tests and bench.py: it marshals numpy arrays and raw
device pointers into the C ABI and nothing else.  All compute happens in the HIP library; when the
library or a GPU is missing every call fails loudly -- there is no CPU fallback here.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import typing
import weakref
from dataclasses import dataclass

import numpy as np

# _abi.py is the one place that knows the C ABI: the structures, the signature table, lib() and EXPORTS
from ._abi import (EXPORTS, LIB_PATH, FheError, _CastParams, _check, _clear, _Handle, _last_error, _nonzero,  # noqa: F401
                   _PackingParams, _Params, _ptr, _record, _u64, lib, seed_bytes)


@dataclass(frozen=True)
class Params:
    """shortint ClassicPBSParameters (reference: tfhe/src/shortint/parameters/mod.rs:61-76)."""
    n: int
    k: int
    N: int
    pbs_base_log: int
    pbs_level: int
    ks_base_log: int
    ks_level: int
    msg_mod: int
    carry_mod: int
    lwe_std: float
    glwe_std: float
    name: str = ""
    grouping: int = 1          # multi-bit PBS grouping factor (1 = classic PBS)

    @property
    def n_ggsw(self) -> int:
        """GGSWs in the bootstrapping key: n (classic) or n/g * 2^g (multi-bit)."""
        return self.n if self.grouping <= 1 else self.n // self.grouping * (1 << self.grouping)

    @property
    def big_size(self) -> int:
        return self.k * self.N + 1

    @property
    def small_size(self) -> int:
        return self.n + 1

    @property
    def glwe_len(self) -> int:
        return (self.k + 1) * self.N

    @property
    def delta(self) -> int:
        return (1 << 63) // (self.msg_mod * self.carry_mod)

    @property
    def ksk_len(self) -> int:
        return self.k * self.N * self.ks_level * (self.n + 1)

    @property
    def bsk_len(self) -> int:
        return self.n_ggsw * self.pbs_level * (self.k + 1) ** 2 * self.N

    def c(self) -> _Params:
        return _Params(self.n, self.k, self.N, self.pbs_base_log, self.pbs_level, self.ks_base_log,
                       self.ks_level, self.msg_mod, self.carry_mod, self.lwe_std, self.glwe_std, self.grouping)


# reference: tfhe/src/shortint/parameters/mod.rs:703-717, :658-672, :613-627
PARAM_MESSAGE_2_CARRY_2_KS_PBS = Params(742, 1, 2048, 23, 1, 3, 5, 4, 4,
                                        0.000007069849454709433, 0.00000000000000029403601535432533,
                                        "PARAM_MESSAGE_2_CARRY_2_KS_PBS")
PARAM_MESSAGE_4_CARRY_4_KS_PBS = Params(996, 1, 32768, 15, 2, 3, 7, 16, 16,
                                        6.767666038309478e-08, 2.168404344971009e-19,
                                        "PARAM_MESSAGE_4_CARRY_4_KS_PBS")
# shortint/parameters/multi_bit.rs:115-135
PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS = Params(818, 1, 2048, 22, 1, 5, 3, 4, 4,
                                                          0.000002226459789930014, 0.0000000000000003152931493498455,
                                                          "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_2_KS_PBS", 2)
# shortint/parameters/multi_bit.rs:173-190
PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS = Params(888, 1, 2048, 21, 1, 7, 2, 4, 4,
                                                          0.0000006125031601933181, 0.0000000000000003152931493498455,
                                                          "PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS", 3)
# shortint/parameters/multi_bit.rs:96-113, :154-171 (N = 512, k = 3) and :134-152, :192-209 (N = 8192, two levels):
# served by the two-kernel path (multibit_combine_generic_kernel + the classic kernels' EXTPROD mode)
PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS = Params(764, 3, 512, 18, 1, 6, 2, 2, 2,
                                                          0.000006025673585415336, 0.0000000000039666089171633006,
                                                          "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_2_KS_PBS", 2)
PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS = Params(765, 3, 512, 18, 1, 6, 2, 2, 2,
                                                          0.000005915594083804978, 0.0000000000039666089171633006,
                                                          "PARAM_MULTI_BIT_MESSAGE_1_CARRY_1_GROUP_3_KS_PBS", 3)
PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS = Params(922, 1, 8192, 14, 2, 4, 4, 8, 8,
                                                          0.0000003272369292345697, 0.0000000000000000002168404344971009,
                                                          "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_2_KS_PBS", 2)
PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS = Params(972, 1, 8192, 14, 2, 6, 3, 8, 8,
                                                          0.00000013016688349592805, 0.0000000000000000002168404344971009,
                                                          "PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3_KS_PBS", 3)
PARAM_MESSAGE_2_CARRY_1_KS_PBS = Params(742, 2, 1024, 23, 1, 4, 3, 4, 2,
                                        0.000007069849454709433, 0.00000000000000029403601535432533,
                                        "PARAM_MESSAGE_2_CARRY_1_KS_PBS")
PARAM_MESSAGE_1_CARRY_1_KS_PBS = Params(684, 3, 512, 18, 1, 4, 3, 2, 2,
                                        0.00002043784477291318, 0.0000000000034525330484572114,
                                        "PARAM_MESSAGE_1_CARRY_1_KS_PBS")


CAST_TO_BIG, CAST_TO_SMALL = 0, 1                      # fhe_cast_params_t.target
CAST_RAW, CAST_REFRESH, CAST_KEYSWITCHED = 0, 1, 2     # the mode of a cast


def random_seed() -> bytes:
    """32 bytes from the OS CSPRNG (fhe_random_seed)."""
    buf = (C.c_uint8 * 32)()
    _check(lib().fhe_random_seed(buf))
    return bytes(buf)


def chacha20_block(key: bytes, counter: int, stream: int) -> np.ndarray:
    out = np.zeros(16, dtype=np.uint32)
    kb = (C.c_uint8 * 32)(*seed_bytes(key))
    _check(lib().fhe_chacha20_block(kb, C.c_uint64(counter), C.c_uint64(stream), _ptr(out)))
    return out


def debug_det_log(x) -> np.ndarray:
    """det_log (csrc/det_math.h, the sampler's libm-free logarithm) of every x, as the host computes it.  Tests only."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.shape, dtype=np.float64)
    _check(lib().fhe_debug_det_log(_ptr(x), x.size, _ptr(out)))
    return out


def debug_noise_samples(seed, stream: int, std_dev: float, count: int) -> np.ndarray:
    """`count` consecutive gaussian_torus values (csrc/det_math.h) of one ChaCha20 stream, as torus words.  Tests only."""
    out = np.zeros(count, dtype=np.uint64)
    sb = (C.c_uint8 * 32)(*seed_bytes(seed))
    _check(lib().fhe_debug_noise_samples(sb, C.c_uint64(stream), float(std_dev), count, _ptr(out)))
    return out


def debug_round_torus(x):
    """(round_half_away(x), from_torus_exact(x)) of every x (csrc/det_math.h).  Tests only."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rounded = np.zeros(x.shape, dtype=np.float64)
    torus = np.zeros(x.shape, dtype=np.uint64)
    _check(lib().fhe_debug_round_torus(_ptr(x), x.size, _ptr(rounded), _ptr(torus)))
    return rounded, torus


def pinned_empty(shape, dtype=np.uint64):
    """numpy array in page-locked host memory (fhe_host_alloc): host <-> GPU copies of it run at the full PCIe rate and
    never page-fault.  Freed when the array (and every view of it) is gone."""
    shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if shape else 1
    ptr = C.c_void_p()
    _check(lib().fhe_host_alloc(max(1, n * dt.itemsize), C.byref(ptr)))
    buf = (C.c_uint8 * max(1, n * dt.itemsize)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    weakref.finalize(buf, lib().fhe_host_free, C.c_void_p(ptr.value))
    return arr


def params_supported(params: "Params"):
    """(True, "") if fhe_engine_create would accept the parameters, else (False, reason).  Needs no device."""
    if lib().fhe_params_supported(C.byref(params.c())) == 0:
        return True, ""
    return False, _last_error()


def noise_model_is_calibrated(params: "Params") -> bool:
    """Has the model's V_pbs been checked against measured PBS output noise for this (N, k, level, grouping) shape?"""
    return bool(lib().fhe_noise_model_is_calibrated(C.byref(params.c())))


def noise_model(params: "Params") -> dict:
    """Variance model of one KS -> PBS (csrc/noise_model.h): variances with the torus = 1."""
    a = _record(C.c_double, 6, lib().fhe_noise_model, C.byref(params.c()))
    return dict(zip(("v_pbs", "v_ks", "v_ms", "half_box", "budget", "log2_pfail_at_budget"), a))


def regex_check(regex) -> dict:
    """Parse a pattern of FheStringOps.matches without building anything: {"positions": character positions of the
    expanded pattern, "max_len": the longest match in characters, None when unbounded}.  Raises FheError with the reason
    (a malformed pattern: with the byte offset)."""
    regex = regex.encode() if isinstance(regex, str) else bytes(regex)
    m, longest = C.c_uint32(0), C.c_uint32(0)
    _check(lib().fhe_regex_check(*_clear(regex), C.byref(m), C.byref(longest)))
    return {"positions": m.value, "max_len": None if longest.value == 0xFFFFFFFF else longest.value}


def kernel_revision() -> str:
    return lib().fhe_kernel_revision().decode()


# ---- transciphering (include/fhestr.h, "transciphering"; csrc/stream_cipher.h, csrc/transcipher.h) ----
TRIVIUM, KREYVIUM = 1, 2          # FHE_STREAM_TRIVIUM, FHE_STREAM_KREYVIUM
_STREAM_CIPHERS = {"trivium": TRIVIUM, "kreyvium": KREYVIUM, TRIVIUM: TRIVIUM, KREYVIUM: KREYVIUM}


def _cipher_id(cipher) -> int:
    try:
        return _STREAM_CIPHERS[cipher.lower() if isinstance(cipher, str) else int(cipher)]
    except (KeyError, ValueError, TypeError):
        raise FheError(f"unknown stream cipher {cipher!r}: 'trivium' or 'kreyvium'") from None


def stream_cipher_info(cipher) -> dict:
    """{"key_bits", "iv_bits", "warmup_steps"} of 'trivium' (80-bit: for its published vectors and parity with the
    reference) or 'kreyvium' (128-bit: the one that matches the 128-bit parameter sets)."""
    return dict(zip(("key_bits", "iv_bits", "warmup_steps"), _record(C.c_uint32, 3, lib().fhe_stream_cipher_info, _cipher_id(cipher))))


def _cipher_bytes(cipher, what: str, b) -> np.ndarray:
    n = stream_cipher_info(cipher)["key_bits"] // 8
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    if a.size != n:
        raise FheError(f"a {what} of this cipher is {n} bytes, got {a.size}")
    return np.ascontiguousarray(a)


def stream_key_bits(cipher, key: bytes) -> np.ndarray:
    """The L bits of a key (or IV) in spec order K_1 .. K_L: K_j = x[L - j] with x[8 j + l] = bit l of byte j."""
    return np.unpackbits(_cipher_bytes(cipher, "key", key), bitorder="little")[::-1].astype(np.uint64)


def stream_keystream(cipher, key: bytes, iv: bytes, n_bytes: int, first_byte: int = 0) -> bytes:
    """Keystream bytes first_byte .. first_byte + n_bytes - 1 in the clear (fhe_stream_cipher_keystream; client side)."""
    k, v = _cipher_bytes(cipher, "key", key), _cipher_bytes(cipher, "IV", iv)
    out = np.zeros(max(int(n_bytes), 1), dtype=np.uint8)
    _check(lib().fhe_stream_cipher_keystream(_cipher_id(cipher), _ptr(k), _ptr(v), C.c_uint64(first_byte), _ptr(out), int(n_bytes)))
    return out[:n_bytes].tobytes()


def stream_encrypt(cipher, key: bytes, iv: bytes, data: bytes, offset: int = 0) -> bytes:
    """data XOR the keystream from byte `offset`: encrypts and decrypts.  What a client sends to Transcipher.next; the
    offset of a call's bytes is Transcipher.offset before that call (every call starts on an 8-byte boundary)."""
    ks = np.frombuffer(stream_keystream(cipher, key, iv, len(data), offset), dtype=np.uint8)
    return (np.frombuffer(bytes(data), dtype=np.uint8) ^ ks).tobytes()


def transcipher_supported(params: "Params", cipher):
    """(True, "") if the parameter set can run the cipher homomorphically, else (False, reason).  Needs no device."""
    if lib().fhe_transcipher_supported(C.byref(params.c()), _cipher_id(cipher)) == 0:
        return True, ""
    return False, _last_error()


def transcipher_tables(params: "Params") -> np.ndarray:
    """The lookup tables of a round over the message-and-carry values, (n_tables, msg_mod * carry_mod): f_3, 1 - f_3, f_4,
    1 - f_4, then g_{i,c} at 4 + 2 i + c (csrc/transcipher.h)."""
    n = C.c_uint32(0)
    _check(lib().fhe_transcipher_table(C.byref(params.c()), 0, None, C.byref(n)))
    out = np.zeros((n.value, params.msg_mod * params.carry_mod), dtype=np.uint64)
    for t in range(n.value):
        _check(lib().fhe_transcipher_table(C.byref(params.c()), t, _ptr(out[t]), C.byref(n)))
    return out


def transcipher_ring_len(params: "Params", streams: int) -> int:
    return int(lib().fhe_transcipher_ring_len(C.byref(params.c()), streams))


def _tc_ivs(cipher, ivs, streams: int) -> np.ndarray:
    n = stream_cipher_info(cipher)["key_bits"] // 8
    if isinstance(ivs, np.ndarray):
        a = np.ascontiguousarray(ivs, dtype=np.uint8).reshape(-1)
    else:
        a = np.ascontiguousarray(np.frombuffer(b"".join(bytes(v) for v in ivs), dtype=np.uint8))
    if a.size != streams * n:
        raise FheError(f"{streams} IVs of this cipher are {streams * n} bytes, got {a.size}")
    return a


def _tc_round(params, call, engine, cipher, streams, round, rows, ring, key, ivs, data, m):
    """gather through the host loops (engine None) or the kernel: (pbs_in (S, rows, big), tables (S, rows))."""
    p = params
    if data is not None:
        data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        data = np.ascontiguousarray(data).reshape(streams, -1)
    pbs_in = np.zeros((streams, rows, p.big_size), dtype=np.uint64)
    tables = np.zeros((streams, rows), dtype=np.uint32)
    head = (engine._h,) if engine is not None else (C.byref(p.c()),)
    _check(call(*head, _cipher_id(cipher), streams, round, rows, _ptr(_u64(ring)), _ptr(_u64(key)), _ptr(_tc_ivs(cipher, ivs, streams)),
                _ptr(data) if data is not None else None, data.shape[1] if data is not None else 0, m, _ptr(pbs_in), _ptr(tables)))
    return pbs_in, tables


def transcipher_init_host(params: "Params", cipher, streams: int, key, ivs, ring=None) -> np.ndarray:
    """The ring with the blocks of rounds -1 and -2 written by the host loop (fhe_transcipher_init_host); the other rows as
    `ring` had them (zeros when None).  key: (L, big) rows K_1 .. K_L."""
    ring = np.zeros(transcipher_ring_len(params, streams), dtype=np.uint64) if ring is None else _u64(ring).reshape(-1).copy()
    _check(lib().fhe_transcipher_init_host(C.byref(params.c()), _cipher_id(cipher), streams, _ptr(_u64(key)), _ptr(_tc_ivs(cipher, ivs, streams)), _ptr(ring)))
    return ring


def transcipher_gather_host(params: "Params", cipher, streams: int, round: int, rows: int, ring, key, ivs, data=None, m: int = 0):
    return _tc_round(params, lib().fhe_transcipher_gather_host, None, cipher, streams, round, rows, ring, key, ivs, data, m)


def transcipher_apply_host(params: "Params", cipher, streams: int, round: int, ring, n_bytes: int, m: int, out) -> np.ndarray:
    """`out` ((S * n_bytes * blocks_per_char, big), updated in place and returned) with the blocks of call round m summed in."""
    _check(lib().fhe_transcipher_apply_host(C.byref(params.c()), _cipher_id(cipher), streams, round, _ptr(_u64(ring)), n_bytes, m, _ptr(out)))
    return out


class Engine(_Handle):
    """One GPU's evaluation engine: resident keys + LUTs, batched KS/PBS (mirrors the evaluation
    half of shortint::ServerKey, tfhe/src/shortint/server_key/mod.rs)."""
    _destroy = "fhe_engine_destroy"

    def __init__(self, params: Params, device: int = 0, log2_points: int = 0):
        self.params = params
        self.device = device
        self._h = C.c_void_p()
        self._dependents = weakref.WeakSet()    # what points into this engine and is closed before it: see _adopt
        self.packing_pair = None                # the (base_log, level) given to load_packing_key
        self.ring_packing_pair = None           # ... and to load_ring_packing_key
        _check(lib().fhe_engine_create(C.byref(params.c()), device, C.byref(self._h)))
        if log2_points:
            _check(lib().fhe_engine_set_variant(self._h, log2_points))

    def _adopt(self, obj):
        """close() closes `obj` before the engine goes: what it holds points into the engine.  obj._close_rank orders
        them: the string operations' cached plans (0) go before string programs and their compiled plans (1)."""
        self._dependents.add(obj)

    def _export_buffers(self, export: bool):
        """(bsk, ksk) arrays for the standard-domain keys a loading call also hands back, (None, None) without export."""
        if not export:
            return None, None
        return np.zeros(self.params.bsk_len, dtype=np.uint64), np.zeros(self.params.ksk_len, dtype=np.uint64)

    def load_seeded_keys(self, ksk_seed, ksk_bodies, bsk_seed, bsk_bodies, export: bool = False):
        """A tfhe-rs CompressedServerKey (shortint/server_key/compressed.rs): bodies + two 128-bit compression seeds
        (16 bytes, or ints = Seed(u128)); the masks are expanded on the GPU.  export=True returns (bsk_std, ksk)."""
        p = self.params
        kb, bb = _u64(ksk_bodies), _u64(bsk_bodies)
        if kb.size != p.k * p.N * p.ks_level or bb.size != p.n_ggsw * p.pbs_level * (p.k + 1) * p.N:
            raise FheError("seeded key: body count does not match the parameter set")
        seeds = [(C.c_uint8 * 16).from_buffer_copy(s.to_bytes(16, "little") if isinstance(s, int) else bytes(s))
                 for s in (ksk_seed, bsk_seed)]
        bsk, ksk = self._export_buffers(export)
        _check(lib().fhe_engine_load_seeded_keys(self._h, seeds[0], _ptr(kb), seeds[1], _ptr(bb), _ptr(bsk), _ptr(ksk)))
        return (bsk, ksk) if export else None

    def expand_seeded_lwe(self, seeds, bodies, d_out: int | None = None):
        """Compressed ciphertexts (one 16-byte compression seed and one body each; shortint CompressedCiphertext) ->
        full big-key ciphertexts, masks generated on the GPU.  d_out: device pointer to write them to (count x
        big_size words) instead of returning a host array."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint8).reshape(-1, 16))
        bodies = _u64(bodies)
        if seeds.shape[0] != bodies.size:
            raise FheError("one seed per body")
        out = None if d_out else np.zeros((bodies.size, self.params.big_size), dtype=np.uint64)
        _check(lib().fhe_engine_expand_seeded_lwe(self._h, seeds.ctypes.data_as(C.c_void_p), _ptr(bodies), bodies.size,
                                                  C.c_void_p(d_out) if d_out else None, _ptr(out) if out is not None else None))
        return out

    def expand_compact_list(self, clist, count: int, d_out: int | None = None, d_list: int | None = None):
        """A public-key client's compact ciphertext list (CompactPublicKey.encrypt; shortint CompactCiphertextList) ->
        `count` big-key ciphertexts, written by the GPU (csrc/compact_kernels.hip.h).  d_out: device pointer to write
        them to (count x big_size words: what apply_lookup_table_dev and Plan.run_batch_dev read) instead of returning
        a host array.  d_list: the list is already on the device at this pointer (clist is ignored); then d_out is
        required and the call only enqueues on the engine's stream."""
        if d_list:
            if not d_out:
                raise FheError("expand_compact_list: a device-resident list needs a device destination (d_out)")
            _check(lib().fhe_engine_expand_compact_list_dev(self._h, C.c_void_p(d_list), count, C.c_void_p(d_out)))
            return None
        clist = _u64(clist).reshape(-1)
        if clist.size != compact_list_len(self.params, count):
            raise FheError(f"compact list: {clist.size} words do not hold {count} ciphertexts of this parameter set")
        out = None if d_out else np.zeros((count, self.params.big_size), dtype=np.uint64)
        _check(lib().fhe_engine_expand_compact_list(self._h, _ptr(clist), count, C.c_void_p(d_out) if d_out else None,
                                                    _ptr(out) if out is not None else None))
        return out

    def set_variant(self, selector: int):
        """Blind-rotation variant: log2(points per thread), + 16 for the two-LWEs-per-CU layout; 0 = automatic.  After the
        keys are loaded only variants with the same points per thread (same Fourier key layout) can be chosen."""
        _check(lib().fhe_engine_set_variant(self._h, selector))

    def set_pipeline(self, mode):
        """Throughput modes for back-to-back apply_lookup_table_dev calls (include/fhestr.h, fhe_engine_set_pipeline):
        0 / False off; 1 / True the keyswitch of call k+1 in the shadow of the blind rotation of call k; 2 whole calls
        overlapped on two streams on the two-LWEs-per-CU kernel."""
        _check(lib().fhe_engine_set_pipeline(self._h, int(mode)))

    def pipeline_input_event(self, hip_event: int):
        """The next pipelined apply_lookup_table_dev call's keyswitch waits for this hipEvent_t (e.g.
        torch.cuda.Event().cuda_event after .record()); see fhe_engine_pipeline_input_event."""
        _check(lib().fhe_engine_pipeline_input_event(self._h, C.c_void_p(hip_event)))

    def set_keep_busy(self, on: bool):
        """Small launches carry replicas on the idle CUs so the GPU keeps its clock for the next large one (include/fhestr.h)."""
        _check(lib().fhe_engine_set_keep_busy(self.handle, int(bool(on))))

    def set_cluster_mode(self, mode: int, max_batch: int = 0xFFFFFFFF):
        """N >= 16384: several CUs per LWE (-1 automatic, 0 never, 1 always; include/fhestr.h)."""
        _check(lib().fhe_engine_set_cluster_mode(self._h, mode, max_batch))

    def cluster_info(self) -> int:
        """Clusters the last cluster launch formed (synchronises)."""
        n = C.c_uint32(0)
        _check(lib().fhe_engine_cluster_info(self._h, C.byref(n)))
        return n.value

    KS_KERNELS = ("none", "mfma", "dot4", "dot4_shadow")

    def keyswitch_info(self) -> dict:
        """What the last keyswitch launch ran (fhe_engine_keyswitch_info, include/fhestr.h): kernel ("none", "mfma", "dot4",
        "dot4_shadow"), tile (row tiles or samples per workgroup), chunks of the sum over the input dimension, steps per chunk,
        steps in all, last_chunk (steps of the last chunk), rotation_regs.  Recorded at launch: no synchronisation."""
        kernel, tile, chunks, per_chunk, steps, regs = _record(C.c_uint32, 6, lib().fhe_engine_keyswitch_info, self._h)
        return {"kernel": self.KS_KERNELS[kernel], "tile": tile, "chunks": chunks, "steps_per_chunk": per_chunk, "steps": steps,
                "last_chunk": steps - (chunks - 1) * per_chunk if chunks else 0, "rotation_regs": regs}

    def cluster_fallbacks(self) -> int:
        """How often a multi-CU launch gave up (compute units held by another kernel) and was re-run on the one-workgroup kernel."""
        n = C.c_uint32(0)
        _check(lib().fhe_engine_cluster_fallbacks(self._h, C.byref(n)))
        return n.value

    def set_multibit_combine_max(self, max_batch: int):
        """Multi-bit PBS: batches up to max_batch prepare their GGSWs on the whole GPU first (0 = always fused)."""
        _check(lib().fhe_engine_set_multibit_combine_max(self._h, max_batch))

    def close(self):
        if self._h:
            for obj in sorted(self._dependents, key=lambda o: o._close_rank):
                obj.close()
        super().close()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return int(lib().fhe_engine_stream(self._h) or 0)

    def synchronize(self):
        _check(lib().fhe_engine_synchronize(self._h))

    def set_stream(self, hip_stream: int | None):
        """Launch on a caller-owned stream handle (e.g. torch.cuda.current_stream().cuda_stream; 0 is
        HIP's default stream).  None switches back to the engine's own stream."""
        if hip_stream is None:
            _check(lib().fhe_engine_reset_stream(self._h))
        else:
            _check(lib().fhe_engine_set_stream(self._h, C.c_void_p(hip_stream)))

    def load_keys(self, bsk_std, ksk):
        p = self.params
        bsk_std, ksk = _u64(bsk_std), _u64(ksk)
        if bsk_std.size != p.bsk_len or ksk.size != p.ksk_len:
            raise FheError("key size mismatch")
        _check(lib().fhe_engine_load_keys(self._h, _ptr(bsk_std), _ptr(ksk)))

    def generate_keys(self, glwe_sk, small_sk, seed: int, export: bool = False):
        """KSK + BSK generated on the device from the secret keys (ServerKey::new,
        shortint/engine/server_side.rs:54-160) and installed; export=True also returns the
        standard-domain (bsk, ksk) it generated."""
        p = self.params
        glwe_sk, small_sk = _u64(glwe_sk), _u64(small_sk)
        if glwe_sk.size != p.k * p.N or small_sk.size != p.n:
            raise FheError("secret key size mismatch")
        bsk, ksk = self._export_buffers(export)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_engine_generate_keys(self._h, _ptr(glwe_sk), _ptr(small_sk), sb, _ptr(bsk), _ptr(ksk)))
        return (bsk, ksk) if export else None

    # shortint/server_key/mod.rs:383-399
    def generate_lookup_table(self, f):
        p = self.params
        table = np.array([int(f(i)) for i in range(p.msg_mod * p.carry_mod)], dtype=np.uint64)
        lut_id, deg = C.c_uint32(), C.c_uint64()
        _check(lib().fhe_lut_generate(self._h, _ptr(table), C.byref(lut_id), C.byref(deg)))
        return lut_id.value, deg.value

    # shortint/server_key/bivariate_pbs.rs:71-96,125-130
    def generate_lookup_table_bivariate(self, f, factor=None):
        p = self.params
        factor = factor or p.msg_mod
        return self.generate_lookup_table(
            lambda x: f((x // factor) % p.msg_mod, (x % factor) % p.msg_mod))

    def upload_lut(self, acc) -> int:
        acc = _u64(acc)
        if acc.size != self.params.glwe_len:
            raise FheError("accumulator size mismatch")
        lut_id = C.c_uint32()
        _check(lib().fhe_lut_upload(self._h, _ptr(acc), C.byref(lut_id)))
        return lut_id.value

    def download_lut(self, lut_id: int) -> np.ndarray:
        acc = np.zeros(self.params.glwe_len, dtype=np.uint64)
        _check(lib().fhe_lut_download(self._h, lut_id, _ptr(acc)))
        return acc

    def load_packing_key(self, pp, pksk):
        """Upload a packing keyswitch key (ClientKey.gen_packing_key) and rewrite it into the kernel's digit planes."""
        pksk = _u64(pksk).reshape(-1)
        if pksk.size != _nonzero(packing_key_len(self.params, pp)):
            raise FheError("packing key: size does not match the parameter set and decomposition")
        _check(lib().fhe_engine_load_packing_key(self._h, C.byref(_pp(pp)), _ptr(pksk)))
        self.packing_pair = (int(pp[0]), int(pp[1]))        # what Narrow(bits=None) takes its default width for

    def load_ring_packing_key(self, pp, key):
        """Upload a ring packing key (ClientKey.gen_ring_packing_key) and rewrite it into transformed digit planes
        (csrc/ring_packing_kernels.hip.h).  With no matrix packing key loaded, Engine.pack, packed=True and the refresh
        gate of unpack / unpack_narrow take the ring route; with one loaded they behave as before."""
        key = _u64(key).reshape(-1)
        if key.size != _nonzero(ring_packing_key_len(self.params, pp)):
            raise FheError("ring packing key: size does not match the parameter set and decomposition")
        _check(lib().fhe_engine_load_ring_packing_key(self._h, C.byref(_pp(pp)), _ptr(key)))
        self.ring_packing_pair = (int(pp[0]), int(pp[1]))

    def _ring_route(self) -> bool:
        return self.packing_pair is None and self.ring_packing_pair is not None

    def ring_pack_info(self) -> dict:
        """What the last ring packing call enqueued (fhe_engine_ring_pack_info)."""
        ran, levels, keyswitches, launches, scratch = _record(C.c_uint64, 5, lib().fhe_engine_ring_pack_info, self._h)
        return {"ran": bool(ran), "levels": levels, "keyswitches": keyswitches, "launches": launches, "scratch_bytes": scratch}

    def ring_ntt(self, polys, inverse: bool = False) -> np.ndarray:
        """The device's negacyclic transform mod 2^32 - 2^20 + 1 on its own (fhe_engine_ring_ntt): (count, N) residues -> a new array."""
        out = np.ascontiguousarray(polys, dtype=np.uint32).copy()
        out = out.reshape(-1, out.shape[-1])
        _check(lib().fhe_engine_ring_ntt(self._h, out.shape[1], int(bool(inverse)), _ptr(out), out.shape[0]))
        return out

    def transcipher(self, cipher, key_cts, max_streams: int = 1) -> "Transcipher":
        """A Transcipher for one stream-cipher key on this engine (server keys loaded): key_cts are the encrypted key bits
        of ClientKey.encrypt_stream_key, (L, kN+1) in spec order; up to max_streams strings run in lockstep."""
        return Transcipher(self, cipher, key_cts, max_streams)

    def cast_key(self, cp: "CastParams", key) -> "CastKey":
        """A source client's casting key made resident on this (the destination's) engine (fhe_cast_key_create): the
        CastKey that FheStringOps.cast and CastKey.cast take blocks of that client through.  An engine holds any number."""
        return CastKey(self, cp, key)

    def cast_prepare(self, blocks, shift: int) -> np.ndarray:
        """On the SOURCE client's engine, before a cast to a set with fewer bits per block (cast_rshift = shift < 0): one
        keyswitch + PBS with the table x -> (x << -shift) % (msg_mod * carry_mod), the reference's first half of that cast
        (key_switching_key/mod.rs:128-140).  The destination cannot tell blocks that skipped this step."""
        if shift >= 0:
            raise FheError(f"cast_prepare: only a cast to fewer bits (a negative shift) needs the source's server key, got {shift}")
        M = self.params.msg_mod * self.params.carry_mod
        lut_id, _ = self.generate_lookup_table(lambda x: (x << -shift) % M)
        blocks = _u64(blocks).reshape(-1, self.params.big_size)
        return self.apply_lookup_table(blocks, np.full(blocks.shape[0], lut_id, dtype=np.uint32))

    def transcipher_init(self, cipher, streams: int, key, ivs, ring=None) -> np.ndarray:
        """transcipher_init_host through transcipher_init_kernel."""
        ring = np.zeros(transcipher_ring_len(self.params, streams), dtype=np.uint64) if ring is None else _u64(ring).reshape(-1).copy()
        _check(lib().fhe_engine_transcipher_init(self._h, _cipher_id(cipher), streams, _ptr(_u64(key)), _ptr(_tc_ivs(cipher, ivs, streams)), _ptr(ring)))
        return ring

    def transcipher_gather(self, cipher, streams: int, round: int, rows: int, ring, key, ivs, data=None, m: int = 0):
        """transcipher_gather_host through transcipher_gather_kernel."""
        return _tc_round(self.params, lib().fhe_engine_transcipher_gather, self, cipher, streams, round, rows, ring, key, ivs, data, m)

    def transcipher_apply(self, cipher, streams: int, round: int, ring, n_bytes: int, m: int, out) -> np.ndarray:
        """transcipher_apply_host through transcipher_apply_kernel."""
        _check(lib().fhe_engine_transcipher_apply(self._h, _cipher_id(cipher), streams, round, _ptr(_u64(ring)), n_bytes, m, _ptr(out)))
        return out

    def _packed_route(self, host, dev, args, shape, words, d_in, d_out):
        """The routes of pack / unpack / narrow / unpack_narrow.  host and dev are the two entry points of the call, both
        (engine, source, *args, destination); shape: the output's, in words; words(): the host input, checked.  The
        source is d_in (a device pointer) or the host input, the destination d_out (a device pointer) or an array that
        is returned.  Device to device only enqueues on the engine's stream.  Where one side is on the host and the
        other on the device, the host side is staged through a device tensor: torch's stream is not ordered with the
        engine's, so torch is synchronised before the call and the engine after it."""
        if d_in and d_out:
            return _check(dev(self._h, C.c_void_p(d_in), *args, C.c_void_p(d_out)))
        if not d_in:
            src = words()
            if not d_out:
                out = np.zeros(shape, dtype=np.uint64)
                _check(host(self._h, _ptr(src), *args, _ptr(out)))
                return out
        import torch
        if d_in:
            out = torch.empty(shape, dtype=torch.int64, device=f"cuda:{self.device}")
            d_out = out.data_ptr()
        else:
            out = None
            staged = torch.from_numpy(src.view(np.int64)).to(f"cuda:{self.device}")
            d_in = staged.data_ptr()
        torch.cuda.synchronize()
        _check(dev(self._h, C.c_void_p(d_in), *args, C.c_void_p(d_out)))
        self.synchronize()                                  # `staged` is released on return
        return None if out is None else out.cpu().numpy().view(np.uint64)

    def narrow(self, glwes=None, held: int | None = None, bits: int | None = None, d_in: int | None = None, d_out: int | None = None):
        """Packed GLWEs narrowed to `bits`-bit coefficients on the GPU (csrc/glwe_narrow_kernels.hip.h; the definition:
        include/fhestr.h, "narrow packed results"): the GLWEs of `held` blocks -> narrow_len(params, held, bits) words.
        glwes: a host array (Engine.pack's, a PackedString gives `held` itself) -> returns a NarrowString; or a torch device
        tensor / d_in: the GLWEs where Engine.pack(d_out=...) wrote them.  With d_out the list is written there
        (asynchronous on the engine's stream) and nothing is returned.  bits=None: the operand-grade default for the
        loaded packing key's pair (narrow_default_bits)."""
        p = self.params
        if glwes is not None and hasattr(glwes, "data_ptr"):
            d_in = glwes.data_ptr()
        if held is None:
            held = getattr(glwes, "count", None)
        if held is None:
            raise FheError("narrow: the number of blocks the GLWEs hold is required")
        if bits is None:
            bits = self._default_narrow_bits()
        n_words = narrow_len(p, held, bits)
        if held and not n_words:
            raise FheError(f"narrow: a width of {bits} bits is refused (8 .. 32)")

        def words():
            w = _u64(glwes).reshape(-1)
            if w.size != packed_glwe_len(p, held):
                raise FheError(f"narrow: {w.size} words are not the packed GLWEs of {held} blocks of this parameter set")
            return w

        out = self._packed_route(lib().fhe_engine_narrow_glwes, lib().fhe_engine_narrow_glwes_dev, (held, bits), (max(n_words, 1),),
                                 words, d_in, d_out)
        return None if out is None else NarrowString(out[:n_words], held, held // blocks_per_char(p), bits)

    def widen(self, d_in: int, held: int, bits: int, d_out: int):
        """A narrow list on the device back to full GLWEs on the device (fhe_engine_widen_narrow_dev): d_out receives
        packed_glwe_len(params, held) words, what Engine.unpack(d_in=...) reads.  Asynchronous on the engine's stream."""
        _check(lib().fhe_engine_widen_narrow_dev(self._h, C.c_void_p(d_in), held, bits, C.c_void_p(d_out)))

    def _default_narrow_bits(self) -> int:
        if self._ring_route():
            return ring_narrow_default_bits(self.params, self.ring_packing_pair, operand=True)
        if self.packing_pair is None:
            raise FheError("Narrow(bits=None) takes its width from the packing pair given to load_packing_key; none is loaded")
        return narrow_default_bits(self.params, self.packing_pair, operand=True)

    def unpack_narrow(self, narrow=None, held: int | None = None, bits: int | None = None, count: int | None = None, first: int = 0,
                      refresh: bool = True, d_in: int | None = None, d_out: int | None = None):
        """Blocks first .. first + count - 1 of a narrow list back into big-key LWEs on the GPU, extracted straight from
        the list (narrow_sample_extract_kernel): the rows Engine.unpack gives on the widened GLWEs, with the same meaning of
        refresh, d_in and d_out.  narrow: a NarrowString (which brings held and bits), a host array, or a torch device
        tensor / d_in.  count=None: all blocks from `first` on.  The refresh is judged with narrow_noise for the loaded
        packing key's pair and `bits`."""
        p = self.params
        if narrow is not None and hasattr(narrow, "data_ptr"):
            d_in = narrow.data_ptr()
        held = getattr(narrow, "count", None) if held is None else held
        bits = getattr(narrow, "bits", None) if bits is None else bits
        if held is None or bits is None:
            raise FheError("unpack_narrow: the blocks the list holds and its width are required")
        if count is None:
            count = held - first

        def words():
            w = _u64(narrow).reshape(-1)
            if w.size != narrow_len(p, held, bits):
                raise FheError(f"unpack_narrow: {w.size} words are not the narrow list of {held} blocks at {bits} bits of this parameter set")
            return w

        return self._packed_route(lib().fhe_engine_unpack_narrow, lib().fhe_engine_unpack_narrow_dev,
                                  (held, bits, first, count, int(bool(refresh))), (max(count, 0), p.big_size), words, d_in, d_out)

    def narrow_info(self) -> dict:
        """What the last narrow / unpack_narrow launched (fhe_engine_narrow_info), recorded when it was enqueued: `kernel`
        is "narrow" (then `items` counts the list's words), "extract" (rows) or "widen" (GLWE words)."""
        ran, kernel, items, workgroups, bits = _record(C.c_uint32, 5, lib().fhe_engine_narrow_info, self._h)
        return {"ran": bool(ran), "kernel": {0: None, 1: "narrow", 2: "extract", 3: "widen"}[kernel], "items": items, "workgroups": workgroups, "bits": bits}

    def pack(self, cts=None, count: int | None = None, d_in: int | None = None, d_out: int | None = None):
        """Packing keyswitch on the GPU (csrc/packing_ks_kernels.hip.h): big-key LWEs -> ceil(count / N) GLWEs, LWE j at
        coefficient j % N of GLWE j // N.  cts: a host array (count, kN+1) -> returns (n_glwe, k+1, N); or a torch device
        tensor / d_in + count: the buffer apply_lookup_table_dev or Plan.run_batch_dev wrote, packed where it lies.  With
        d_out the GLWEs are written there (asynchronous on the engine's stream) and nothing is returned; without it
        they come back as a host array.  With only a ring packing key loaded (load_ring_packing_key) the same GLWE
        layout comes from the ring route (csrc/ring_packing_kernels.hip.h)."""
        p = self.params
        if cts is not None and hasattr(cts, "data_ptr"):
            if count is None:
                count = cts.numel() // p.big_size
            d_in = cts.data_ptr()
        if d_in:
            if count is None:
                raise FheError("pack: a device buffer needs a count")
        else:
            cts = _u64(cts).reshape(-1, p.big_size)
            count = cts.shape[0]
        L = lib()
        host, dev = ((L.fhe_engine_ring_pack_lwes, L.fhe_engine_ring_pack_lwes_dev) if self._ring_route() else
                     (L.fhe_engine_pack_lwes, L.fhe_engine_pack_lwes_dev))
        return self._packed_route(host, dev, (count,), (-(-count // p.N), p.k + 1, p.N), lambda: cts, d_in, d_out)

    def packing_info(self) -> dict:
        """What the last pack launch ran (fhe_engine_packing_info): row tiles per workgroup, K chunks, K steps per chunk."""
        ran, tile, chunks, spc, steps = _record(C.c_uint32, 5, lib().fhe_engine_packing_info, self._h)
        return {"ran": bool(ran), "tile": tile, "chunks": chunks, "steps_per_chunk": spc, "steps": steps,
                "last_chunk": steps - (chunks - 1) * spc if ran else 0}

    def unpack(self, glwes=None, count: int | None = None, first: int = 0, refresh: bool = True, d_in: int | None = None,
               d_out: int | None = None):
        """Packed results back into big-key LWEs on the GPU (csrc/glwe_extract_kernels.hip.h): blocks first .. first +
        count - 1 of the GLWEs (block j = coefficient j % N of GLWE j // N, what Engine.pack returns) -> (count, kN+1).
        refresh=True sends them through one keyswitch + PBS with the identity table, after which they carry nominal noise
        and are valid inputs of every plan (needs the server keys and a loaded packing key, whose decomposition decides
        whether the refresh is admissible: packing_unpack_noise); refresh=False returns the raw extracted words.
        glwes: a host array, or a torch device tensor / d_in: the GLWEs where they lie.  With d_out (a device pointer to
        count x big_size words, 8-byte aligned: what Plan.run_dev reads) the call only enqueues on the engine's stream
        and returns nothing.  The GLWEs must hold block first + count - 1."""
        p = self.params
        if glwes is not None and hasattr(glwes, "data_ptr"):
            d_in = glwes.data_ptr()
        if count is None:
            count = getattr(glwes, "count", None)
        if count is None:
            raise FheError("unpack: a block count is required")

        def words():
            w = _u64(glwes).reshape(-1)
            if w.size < packed_glwe_len(p, first + count) or w.size % ((p.k + 1) * p.N):
                raise FheError(f"unpack: {w.size} words do not hold packed block {first + count - 1} of this parameter set")
            return w

        return self._packed_route(lib().fhe_engine_unpack_glwes, lib().fhe_engine_unpack_glwes_dev,
                                  (first, count, int(bool(refresh))), (count, p.big_size), words, d_in, d_out)

    def unpack_info(self) -> dict:
        """What the last unpack launched (fhe_engine_unpack_info), recorded when it was enqueued."""
        ran, rows, workgroups, refreshed = _record(C.c_uint32, 4, lib().fhe_engine_unpack_info, self._h)
        return {"ran": bool(ran), "rows": rows, "workgroups": workgroups, "refreshed": bool(refreshed)}

    def keyswitch(self, cts) -> np.ndarray:
        p = self.params
        cts = _u64(cts).reshape(-1, p.big_size)
        out = np.zeros((cts.shape[0], p.small_size), dtype=np.uint64)
        _check(lib().fhe_keyswitch_batch(self._h, _ptr(cts), _ptr(out), cts.shape[0]))
        return out

    def _idx(self, lut_idx, count):
        if lut_idx is None:
            return None, None
        idx = np.ascontiguousarray(lut_idx, dtype=np.uint32)
        if idx.size != count:
            raise FheError("lut_idx length mismatch")
        return idx, _ptr(idx)

    def pbs(self, cts_small, lut_idx=None) -> np.ndarray:
        p = self.params
        cts_small = _u64(cts_small).reshape(-1, p.small_size)
        out = np.zeros((cts_small.shape[0], p.big_size), dtype=np.uint64)
        idx, ip = self._idx(lut_idx, cts_small.shape[0])
        _check(lib().fhe_pbs_batch(self._h, _ptr(cts_small), ip, _ptr(out), cts_small.shape[0]))
        return out

    def apply_lookup_table(self, cts, lut_idx=None) -> np.ndarray:
        """Batched KS -> PBS (shortint/server_key/mod.rs:457-476,783-857)."""
        p = self.params
        cts = _u64(cts).reshape(-1, p.big_size)
        out = np.zeros_like(cts)
        idx, ip = self._idx(lut_idx, cts.shape[0])
        _check(lib().fhe_ks_pbs_batch(self._h, _ptr(cts), ip, _ptr(out), cts.shape[0]))
        return out

    def apply_lookup_table_small_key(self, cts_small, lut_idx=None) -> np.ndarray:
        """PBS -> KS order on small-key ciphertexts (shortint/server_key/mod.rs:859-932)."""
        p = self.params
        cts_small = _u64(cts_small).reshape(-1, p.small_size)
        out = np.zeros_like(cts_small)
        idx, ip = self._idx(lut_idx, cts_small.shape[0])
        _check(lib().fhe_pbs_ks_batch(self._h, _ptr(cts_small), ip, _ptr(out), cts_small.shape[0]))
        return out

    def apply_lookup_table_dev(self, d_in: int, d_lut_idx: int | None, d_out: int, count: int):
        """Device-pointer variant, asynchronous on the engine stream."""
        _check(lib().fhe_ks_pbs_batch_dev(self._h, C.c_void_p(d_in),
                                          C.c_void_p(d_lut_idx) if d_lut_idx else None,
                                          C.c_void_p(d_out), count))

    def lincomb(self, pool, jobs):
        """jobs: list of (terms=[(src, coeff), ...], const_body)."""
        p = self.params
        pool = _u64(pool).reshape(-1, p.big_size)
        off = np.zeros(len(jobs) + 1, dtype=np.uint32)
        src, coeff, cst = [], [], []
        for j, (terms, c) in enumerate(jobs):
            for s, a in terms:
                src.append(s)
                coeff.append(a)
            off[j + 1] = len(src)
            cst.append(c & (2 ** 64 - 1))
        src = np.array(src + [0], dtype=np.uint32)
        coeff = np.array(coeff + [0], dtype=np.int32)
        cst = np.array(cst, dtype=np.uint64)
        out = np.zeros((len(jobs), p.big_size), dtype=np.uint64)
        _check(lib().fhe_lwe_lincomb_batch(self._h, _ptr(pool), pool.shape[0], _ptr(off), _ptr(src),
                                           _ptr(coeff), _ptr(cst), _ptr(out), len(jobs)))
        return out

    def last_kernel_ms(self):
        return tuple(_record(C.c_float, 2, lib().fhe_last_kernel_ms, self._h))

    def kernel_times(self, reset=True):
        """(keyswitch_ms_total, blind_rotate_ms_total, calls) since the last reset (HIP events)."""
        ms = (C.c_double * 2)()
        calls = C.c_uint32()
        _check(lib().fhe_kernel_times(self._h, ms, C.byref(calls), 1 if reset else 0))
        return float(ms[0]), float(ms[1]), int(calls.value)


class Transcipher(_Handle):
    """Strings encrypted under Trivium / Kreyvium turned into encrypted strings on the GPU (fhe_transcipher_*):
    begin(ivs) runs the warm-up of one string per IV, next(data) returns the next characters of each as the block
    ciphertexts FheStringOps and StringProgram take.  Every next starts on an 8-byte keystream boundary: `offset` is
    the keystream byte the coming call starts at, which the client passes to stream_encrypt for that call's bytes."""
    _destroy, _engine_owned = "fhe_transcipher_destroy", True

    def __init__(self, engine: "Engine", cipher, key_cts, max_streams: int = 1):
        self.engine, self.cipher, self.params = engine, _cipher_id(cipher), engine.params
        key_cts = _u64(key_cts).reshape(-1)
        L = stream_cipher_info(cipher)["key_bits"]
        if key_cts.size != L * self.params.big_size:
            raise FheError(f"transcipher: {L} key-bit ciphertexts of {self.params.big_size} words expected, got {key_cts.size} words")
        self._h = C.c_void_p()
        _check(lib().fhe_transcipher_create(engine._h, self.cipher, _ptr(key_cts), max_streams, C.byref(self._h)))
        self.max_streams, self.streams = max_streams, 0

    def begin(self, ivs):
        """ivs: one IV (bytes) per string, at most max_streams."""
        ivs = [ivs] if isinstance(ivs, (bytes, bytearray)) else list(ivs)
        _check(lib().fhe_transcipher_begin(self._h, _ptr(_tc_ivs(self.cipher, ivs, len(ivs))), len(ivs)))
        self.streams = len(ivs)
        return self

    def next(self, data, refresh: bool = True, d_out: int | None = None):
        """data: the clear cipher bytes, one equally long bytes object per string (or one for a single string).  Returns
        (streams, n_bytes * blocks_per_char, kN+1) block ciphertexts, a single string squeezed to 2-D like
        encrypt_string's; with d_out (a device pointer with room for them) they are written there, asynchronously on the
        engine's stream, and nothing is returned."""
        single = isinstance(data, (bytes, bytearray))
        rows = [bytes(data)] if single else [bytes(d) for d in data]
        if self.streams and (len(rows) != self.streams or len({len(r) for r in rows}) != 1):
            raise FheError(f"transcipher: next takes {self.streams} equally long byte strings")
        n = len(rows[0])
        buf = np.ascontiguousarray(np.frombuffer(b"".join(rows), dtype=np.uint8))
        if not self.streams:                    # the library's own refusal: next before begin
            _check(lib().fhe_transcipher_next(self._h, _ptr(buf), n, int(bool(refresh)), None, None))
        if d_out:
            _check(lib().fhe_transcipher_next(self._h, _ptr(buf), n, int(bool(refresh)), None, C.c_void_p(d_out)))
            return None
        out = np.zeros((self.streams, n * blocks_per_char(self.params), self.params.big_size), dtype=np.uint64)
        _check(lib().fhe_transcipher_next(self._h, _ptr(buf), n, int(bool(refresh)), _ptr(out), None))
        return out[0] if single else out

    def info(self) -> dict:
        v = _record(C.c_uint32, 8, lib().fhe_transcipher_info, self._h)
        return {"cipher": v[0], "max_streams": v[1], "streams": v[2], "warmup_rounds": v[3], "data_rounds": v[4], "pbs": v[5] | (v[6] << 32), "offset": v[7]}

    @property
    def offset(self) -> int:
        return self.info()["offset"]

    def timing(self, on: bool = True) -> dict:
        """Switch the per-phase timing of data rounds on or off and return what was measured since begin: ms of the gather,
        keyswitch + PBS and apply phases and the rounds they cover.  Measurement only: a timed round synchronises."""
        ms, n = (C.c_double * 3)(), C.c_uint32(0)
        _check(lib().fhe_transcipher_timing(self._h, int(bool(on)), ms, C.byref(n)))
        return {"gather_ms": ms[0], "ks_pbs_ms": ms[1], "apply_ms": ms[2], "rounds": n.value}


class ClientKey(_Handle):
    """Client side (CPU): mirrors shortint::ClientKey (tfhe/src/shortint/client_key/mod.rs)."""
    _destroy = "fhe_client_key_destroy"

    def __init__(self, params: Params, seed):
        """seed: 32 bytes (random_seed()) or, for reproducible tests, an int."""
        self.params = params
        self._h = C.c_void_p()
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_client_key_create(C.byref(params.c()), sb, C.byref(self._h)))

    def encrypt(self, msgs) -> np.ndarray:
        msgs = _u64(np.atleast_1d(msgs))
        cts = np.zeros((msgs.size, self.params.big_size), dtype=np.uint64)
        _check(lib().fhe_client_encrypt(self._h, _ptr(msgs), msgs.size, _ptr(cts)))
        return cts

    def decrypt(self, cts) -> np.ndarray:
        """message-and-carry value of every ciphertext."""
        cts = _u64(cts).reshape(-1, self.params.big_size)
        out = np.zeros(cts.shape[0], dtype=np.uint64)
        _check(lib().fhe_client_decrypt(self._h, _ptr(cts), cts.shape[0], _ptr(out)))
        return out.astype(np.int64)

    def encrypt_stream_key(self, cipher, key: bytes) -> np.ndarray:
        """The key bits of a stream-cipher key as ciphertexts of 0 / 1, (L, kN+1) in spec order K_1 .. K_L: what
        Engine.transcipher takes.  Uploaded once per key; the strings then travel as stream_encrypt's bytes."""
        return self.encrypt(stream_key_bits(cipher, key))

    def gen_server_keys(self, threads: int | None = None):
        p = self.params
        bsk = np.zeros(p.bsk_len, dtype=np.uint64)
        ksk = np.zeros(p.ksk_len, dtype=np.uint64)
        _check(lib().fhe_client_gen_server_keys(self._h, _ptr(bsk), _ptr(ksk),
                                                threads or min(16, os.cpu_count() or 1)))
        return bsk, ksk

    def compact_public_key(self, seed) -> "CompactPublicKey":
        """The compact public key of this client's big key (shortint CompactPublicKey::new); `seed` (32 bytes or an
        int) drives its mask and noise.  Refused when k*N is not a power of two."""
        p = self.params
        n = compact_pk_len(p)
        if not n:
            raise FheError(f"a compact public key needs a power-of-two encryption key dimension, k*N = {p.k * p.N}")
        pk = np.zeros(n, dtype=np.uint64)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_client_gen_compact_public_key(self._h, sb, _ptr(pk)))
        return CompactPublicKey(p, pk)

    def gen_packing_key(self, pp=None, seed=0, threads: int | None = None):
        """Packing keyswitch key for this client's keys (fhe_client_gen_packing_key): returns ((base_log, level), words).
        pp=None takes packing_default_params.  `seed` (32 bytes or an int) drives its masks and noise."""
        p = self.params
        pp = tuple(pp) if pp is not None else packing_default_params(p)
        pksk = np.zeros(_nonzero(packing_key_len(p, pp)), dtype=np.uint64)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_client_gen_packing_key(self._h, C.byref(_pp(pp)), sb, _ptr(pksk), threads or min(16, os.cpu_count() or 1)))
        return pp, pksk

    def gen_ring_packing_key(self, pair=None, seed=0, threads: int | None = None):
        """Ring packing key for this client's keys (fhe_client_gen_ring_packing_key): log2(N) automorphism keys of
        k * level GLWE ciphertexts each; returns ((base_log, level), words).  pair=None takes ring_packing_default_params."""
        p = self.params
        pair = tuple(pair) if pair is not None else ring_packing_default_params(p)
        key = np.zeros(_nonzero(ring_packing_key_len(p, pair)), dtype=np.uint64)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_client_gen_ring_packing_key(self._h, C.byref(_pp(pair)), sb, _ptr(key), threads or min(16, os.cpu_count() or 1)))
        return pair, key

    def gen_cast_key(self, dst_ck: "ClientKey", target: int = CAST_TO_SMALL, pair=None, seed=0):
        """The key that takes THIS client's blocks to dst_ck's engine (fhe_client_gen_cast_key; shortint::KeySwitchingKey):
        returns (CastParams, words) for Engine.cast_key on the destination's engine.  target: CAST_TO_BIG, the
        reference's form with the default pair (1, 15), or CAST_TO_SMALL, to the destination's small key with its own
        keyswitch pair.  pair=(base_log, level) overrides the default."""
        cp = cast_default_params(self.params, dst_ck.params, target, pair)
        n = cast_key_len(dst_ck.params, cp)
        key = np.zeros(n, dtype=np.uint64)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_client_gen_cast_key(self._h, dst_ck._h, C.byref(cp.c()), sb, _ptr(key)))
        return cp, key

    def decrypt_packed(self, glwes, count: int) -> np.ndarray:
        """message-and-carry value of the first `count` coefficients of packed results (Engine.pack)."""
        glwes = _u64(glwes).reshape(-1)
        if glwes.size != packed_glwe_len(self.params, count):
            raise FheError(f"decrypt_packed: {glwes.size} words do not hold {count} packed ciphertexts of this parameter set")
        out = np.zeros(count, dtype=np.uint64)
        _check(lib().fhe_client_decrypt_packed(self._h, _ptr(glwes), count, _ptr(out)))
        return out.astype(np.int64)

    def decrypt_narrow(self, narrow, held: int | None = None, bits: int | None = None) -> np.ndarray:
        """message-and-carry value of the `held` blocks of a narrow list (Engine.narrow, packed=Narrow()): the phase of the
        widened GLWEs, decoded like decrypt_packed.  A NarrowString brings held and bits itself."""
        held = getattr(narrow, "count", None) if held is None else held
        bits = getattr(narrow, "bits", None) if bits is None else bits
        if held is None or bits is None:
            raise FheError("decrypt_narrow: the blocks the list holds and its width are required")
        narrow = _u64(narrow).reshape(-1)
        if narrow.size != narrow_len(self.params, held, bits):
            raise FheError(f"decrypt_narrow: {narrow.size} words are not the narrow list of {held} blocks at {bits} bits of this parameter set")
        out = np.zeros(held, dtype=np.uint64)
        _check(lib().fhe_client_decrypt_narrow(self._h, _ptr(narrow), held, bits, _ptr(out)))
        return out.astype(np.int64)

    def secret_keys(self):
        p = self.params
        g = np.zeros(p.k * p.N, dtype=np.uint64)
        s = np.zeros(p.n, dtype=np.uint64)
        _check(lib().fhe_client_secret_keys(self._h, _ptr(g), _ptr(s)))
        return g, s


@dataclass(frozen=True)
class CastParams:
    """fhe_cast_params_t: the source client's parameter set, the cast key's decomposition and its target."""
    src: Params
    base_log: int
    level: int
    target: int

    def c(self) -> _CastParams:
        return _CastParams(self.src.c(), int(self.base_log), int(self.level), int(self.target))


def cast_default_params(src: Params, dst: Params, target: int = CAST_TO_SMALL, pair=None) -> CastParams:
    """The casting key's parameters from src to dst (fhe_cast_default_params): (1, 15) for CAST_TO_BIG, the destination's
    own keyswitch pair for CAST_TO_SMALL, or `pair`.  Raises with the reason for a refused combination."""
    out = _CastParams()
    if pair is None:
        _check(lib().fhe_cast_default_params(C.byref(src.c()), C.byref(dst.c()), int(target), C.byref(out)))
        return CastParams(src, int(out.base_log), int(out.level), int(target))
    cp = CastParams(src, int(pair[0]), int(pair[1]), int(target))
    cast_key_len(dst, cp)
    return cp


def cast_key_len(dst: Params, cp: CastParams) -> int:
    """u64 words of the casting key (fhe_cast_key_len); raises with the reason when the parameters are refused."""
    return _nonzero(lib().fhe_cast_key_len(C.byref(dst.c()), C.byref(cp.c())))


def cast_rshift(src: Params, dst: Params) -> int:
    """log2 of dst's msg_mod * carry_mod minus log2 of src's (fhe_cast_rshift; key_switching_key/mod.rs:62-80)."""
    out = C.c_int32()
    _check(lib().fhe_cast_rshift(C.byref(src.c()), C.byref(dst.c()), C.byref(out)))
    return int(out.value)


def cast_regroup_check(src: Params, dst: Params, group: int) -> tuple:
    """(largest lookup input, the destination's msg_mod * carry_mod) of regrouping `group` source blocks into one
    destination block, (msg_src^group - 1) << cast_rshift (fhe_cast_regroup_check); raises with the reason when refused."""
    degree, space = C.c_uint64(), C.c_uint64()
    _check(lib().fhe_cast_regroup_check(C.byref(src.c()), C.byref(dst.c()), int(group), C.byref(degree), C.byref(space)))
    return int(degree.value), int(space.value)


def cast_out_size(dst: Params, cp: CastParams) -> int:
    """Words of a keyswitched row: the destination's k N + 1 (CAST_TO_BIG) or n + 1 (CAST_TO_SMALL)."""
    return (dst.n if cp.target == CAST_TO_SMALL else dst.k * dst.N) + 1


def cast_host(dst: Params, cp: CastParams, key, cts) -> np.ndarray:
    """The cast's keyswitch as a plain CPU loop (fhe_cast_host): (count, src kN+1) -> (count, cast_out_size).  Bit-identical
    to CastKey.cast(..., mode=CAST_KEYSWITCHED)."""
    cts = _u64(cts).reshape(-1, cp.src.big_size)
    key = _u64(key).reshape(-1)
    if key.size != cast_key_len(dst, cp):
        raise FheError(f"cast_host: {key.size} words are not the casting key of these parameters")
    out = np.zeros((cts.shape[0], cast_out_size(dst, cp)), dtype=np.uint64)
    _check(lib().fhe_cast_host(C.byref(dst.c()), C.byref(cp.c()), _ptr(key), _ptr(cts), cts.shape[0], _ptr(out)))
    return out


def cast_noise(dst: Params, cp: CastParams, v_in: float = 1.0) -> tuple:
    """(what the destination's next lookup sees of a keyswitched block, in its nominal units; its PBS-input budget; the
    keyswitched block's variance with the torus as unit) for a source block of v_in source-nominal variances: fhe_cast_noise."""
    return tuple(_record(C.c_double, 3, lib().fhe_cast_noise, C.byref(dst.c()), C.byref(cp.c()), float(v_in)))


class CastKey(_Handle):
    """One source client's casting key resident on the destination's engine (fhe_cast_key_*; Engine.cast_key).  cast and
    cast_packed take that client's blocks -- rows, or packed GLWEs as they are stored -- to blocks of the engine's client."""
    _destroy, _engine_owned = "fhe_cast_key_destroy", True

    def __init__(self, engine: "Engine", cp: CastParams, key):
        self.engine, self.cp, self.params = engine, cp, engine.params
        key = _u64(key).reshape(-1)
        if key.size != cast_key_len(engine.params, cp):
            raise FheError(f"cast_key: {key.size} words are not the casting key of these parameters")
        self._h = C.c_void_p()
        _check(lib().fhe_cast_key_create(engine._h, C.byref(cp.c()), _ptr(key), C.byref(self._h)))
        self.shift = cast_rshift(cp.src, engine.params)
        self.group, self.v_in = 1, 1.0

    def info(self) -> dict:
        v = _record(C.c_uint32, 8, lib().fhe_cast_key_info, self._h)
        return {"target": v[0], "base_log": v[1], "level": v[2], "in_dim": v[3], "out_dim": v[4], "shift": v[5] - 64, "fused": bool(v[6]),
                "last": {0: None, 1: "lwes", 2: "fused", 3: "extract"}[v[7]]}

    def set_fused(self, on: bool):
        """Packed inputs through cast_decompose_glwe_kernel (default) or through extraction + ks_decompose_kernel."""
        _check(lib().fhe_cast_key_set_fused(self._h, int(bool(on))))

    def set_group(self, group: int):
        """`group` source blocks into one destination block (fhe_cast_key_set_group); 1 switches regrouping off."""
        _check(lib().fhe_cast_key_set_group(self._h, int(group)))
        self.group = int(group)

    def set_input_noise(self, v_in: float):
        """Declare what the source blocks carry, in the source's nominal units (fhe_cast_key_set_input_noise): 1 for stored
        results (the default), 0 for fresh encryptions.  The refusal of a cast that ends in a table judges by it."""
        _check(lib().fhe_cast_key_set_input_noise(self._h, float(v_in)))
        self.v_in = float(v_in)

    def _out_shape(self, count, mode, group):
        if mode == CAST_KEYSWITCHED:
            return (count, cast_out_size(self.params, self.cp))
        return (count // group, self.params.big_size)

    @contextlib.contextmanager
    def _settings(self, group, v_in):
        """`group` and `v_in` of ONE call: the handle's settings are put back when the call has been enqueued, so a later
        call on the same key does not inherit them.  None leaves the handle's own setting."""
        old_group, old_v = self.group, self.v_in
        try:
            if group is not None and group != old_group:
                self.set_group(group)
            if v_in is not None and v_in != old_v:
                self.set_input_noise(v_in)
            yield self.group
        finally:
            if self.group != old_group:
                self.set_group(old_group)
            if self.v_in != old_v:
                self.set_input_noise(old_v)

    def cast(self, cts, mode: int = CAST_REFRESH, d_out: int | None = None, count: int | None = None, group: int | None = None,
             v_in: float | None = None):
        """Source blocks (count, src kN+1) -> destination blocks (fhe_cast_lwes).  mode: CAST_RAW (the reference's
        behaviour: no table where the bits per block agree), CAST_REFRESH (the identity table then), CAST_KEYSWITCHED (the
        keyswitched rows alone).  cts may be a torch device tensor with d_out a device pointer: asynchronous on the
        engine's stream (fhe_cast_lwes_dev), nothing is returned.  group / v_in: regrouping and declared input noise of
        this call alone (set_group, set_input_noise)."""
        with self._settings(group, v_in) as g:
            if hasattr(cts, "data_ptr"):
                count = cts.numel() // self.cp.src.big_size if count is None else count
                _check(lib().fhe_cast_lwes_dev(self._h, C.c_void_p(cts.data_ptr()), count, mode, C.c_void_p(d_out)))
                return None
            cts = _u64(cts).reshape(-1, self.cp.src.big_size)
            out = np.zeros(self._out_shape(cts.shape[0], mode, g), dtype=np.uint64)
            _check(lib().fhe_cast_lwes(self._h, _ptr(cts), cts.shape[0], mode, _ptr(out)))
            return out

    def cast_packed(self, glwes, count: int | None = None, first: int = 0, mode: int = CAST_REFRESH, d_out: int | None = None,
                    group: int | None = None, v_in: float | None = None):
        """Blocks first .. first + count - 1 of the source's packed GLWEs -> destination blocks (fhe_cast_packed): the
        digits are taken straight from the GLWEs, the blocks are never unpacked under the old key.  A PackedString brings
        its count; a torch device tensor with d_out runs asynchronously (fhe_cast_packed_dev).  v_in: what a packed block
        carries, packing_unpack_noise(source set, source's packing pair)[0] for a packed lookup output."""
        if count is None:
            count = getattr(glwes, "count", None)
        if count is None:
            raise FheError("cast_packed: a block count is required")
        with self._settings(group, v_in) as g:
            if hasattr(glwes, "data_ptr"):
                _check(lib().fhe_cast_packed_dev(self._h, C.c_void_p(glwes.data_ptr()), first, count, mode, C.c_void_p(d_out)))
                return None
            src = self.cp.src
            glwes = _u64(glwes).reshape(-1)
            if glwes.size < packed_glwe_len(src, first + count) or glwes.size % src.glwe_len:
                raise FheError(f"cast_packed: {glwes.size} words do not hold packed block {first + count - 1} of the source parameter set")
            out = np.zeros(self._out_shape(count, mode, g), dtype=np.uint64)
            _check(lib().fhe_cast_packed(self._h, _ptr(glwes), first, count, mode, _ptr(out)))
            return out

    def cast_narrow(self, narrow, held: int | None = None, bits: int | None = None, count: int | None = None, first: int = 0,
                    mode: int = CAST_REFRESH, d_out: int | None = None, group: int | None = None, v_in: float | None = None):
        """Blocks first .. first + count - 1 of the source's narrow list -> destination blocks (fhe_cast_narrow): the list
        goes up as it is stored, is widened on the GPU at the source's shape and cast as packed GLWEs.  A NarrowString
        brings held and bits; a torch device tensor with d_out runs asynchronously (fhe_cast_narrow_dev).  v_in: what such
        a block carries, narrow_noise(source set, source's packing pair, bits)[0] for a packed lookup output."""
        held = getattr(narrow, "count", None) if held is None else held
        bits = getattr(narrow, "bits", None) if bits is None else bits
        if held is None or bits is None:
            raise FheError("cast_narrow: the blocks the list holds and its width are required")
        count = held - first if count is None else count
        with self._settings(group, v_in) as g:
            if hasattr(narrow, "data_ptr"):
                _check(lib().fhe_cast_narrow_dev(self._h, C.c_void_p(narrow.data_ptr()), held, bits, first, count, mode, C.c_void_p(d_out)))
                return None
            words = _narrow_words("cast_narrow", self.cp.src, narrow, held, bits)
            out = np.zeros(self._out_shape(count, mode, g), dtype=np.uint64)
            _check(lib().fhe_cast_narrow(self._h, _ptr(words), held, bits, first, count, mode, _ptr(out)))
            return out

    def digits(self, src, count: int, first: int = 0, packed: bool = False) -> np.ndarray:
        """The batch's digit fragments as the product reads them (fhe_cast_debug_digits): int8, for tests."""
        n = C.c_size_t(0)
        src = _u64(src).reshape(-1)
        _check(lib().fhe_cast_debug_digits(self._h, None, first, count, int(packed), None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int8)
        _check(lib().fhe_cast_debug_digits(self._h, _ptr(src), first, count, int(packed), _ptr(out), C.byref(n)))
        return out


def _pp(pp) -> _PackingParams:
    base_log, level = pp
    return _PackingParams(int(base_log), int(level))


def packing_default_params(params: Params):
    """(base_log, level) of the cheapest packing keyswitch key whose packed results still decode within the failure bound
    plans enforce (fhe_packing_default_params).  Raises for parameter sets whose key would exceed 4 GiB."""
    out = _PackingParams()
    _check(lib().fhe_packing_default_params(C.byref(params.c()), C.byref(out)))
    return int(out.base_log), int(out.level)


def packing_key_len(params: Params, pp) -> int:
    """Words of a packing keyswitch key k N * level * (k+1) N; 0 = this (parameter set, decomposition) is refused."""
    return int(lib().fhe_packing_key_len(C.byref(params.c()), C.byref(_pp(pp))))


def ring_packing_default_params(params: Params):
    """(base_log, level) of the cheapest ring packing key -- fewest levels, then largest base, under the one-prime bound --
    whose packed results still decode within the failure bound plans enforce (fhe_ring_packing_default_params)."""
    out = _PackingParams()
    _check(lib().fhe_ring_packing_default_params(C.byref(params.c()), C.byref(out)))
    return (int(out.base_log), int(out.level))


def ring_packing_key_len(params: Params, pair) -> int:
    """Words of a ring packing key log2(N) * k * level * (k+1) N; 0 = this (parameter set, pair) is refused."""
    return int(lib().fhe_ring_packing_key_len(C.byref(params.c()), C.byref(_pp(pair))))


def ring_packing_noise(params: Params, pair) -> tuple:
    """(variance of a raw block extracted from a ring-packed PBS output, in nominal units; the default PBS-input budget)."""
    return tuple(_record(C.c_double, 2, lib().fhe_ring_packing_noise, C.byref(params.c()), C.byref(_pp(pair))))


def ring_narrow_noise(params: Params, pair, bits: int) -> tuple:
    """narrow_noise for the ring route (fhe_ring_narrow_noise)."""
    return tuple(_record(C.c_double, 3, lib().fhe_ring_narrow_noise, C.byref(params.c()), C.byref(_pp(pair)), bits))


def ring_narrow_default_bits(params: Params, pair, operand: bool = True) -> int:
    """narrow_default_bits for the ring route: the smallest width of 8 .. 32 bits whose list may come back as an operand
    (out[0] <= out[1] of ring_narrow_noise).  Only the operand grade is offered."""
    if not operand:
        raise FheError("ring_narrow_default_bits: only the operand grade is offered; choose a client-grade width with ring_narrow_noise")
    for bits in range(8, 33):
        v = ring_narrow_noise(params, pair, bits)
        if v[0] <= v[1]:
            return bits
    raise FheError(f"narrow: no width of 8 .. 32 bits is operand-grade under the ring packing pair {tuple(pair)}")


def ring_pack_keyswitches(params: Params, count: int) -> int:
    """Automorphism keyswitches of ring-packing `count` LWEs: per GLWE of c blocks, sum over d < log2 N of min(2^d, c)."""
    return int(lib().fhe_ring_pack_keyswitches(C.byref(params.c()), count))


def ring_pack_host(params: Params, pair, key, cts) -> np.ndarray:
    """Ring packing on the CPU (fhe_ring_pack_host): cts (count, kN+1) -> (ceil(count / N), k+1, N).  Bit-identical to
    Engine.pack on the ring route."""
    key = _u64(key).reshape(-1)
    cts = _u64(cts).reshape(-1, params.big_size)
    if key.size != ring_packing_key_len(params, pair) or not key.size:
        raise FheError(_last_error() if not ring_packing_key_len(params, pair) else "ring packing key: size does not match the parameter set")
    out = np.zeros((-(-cts.shape[0] // params.N), params.k + 1, params.N), dtype=np.uint64)
    _check(lib().fhe_ring_pack_host(C.byref(params.c()), C.byref(_pp(pair)), _ptr(key), _ptr(cts), cts.shape[0], _ptr(out)))
    return out


def ring_ntt_host(polys, inverse: bool = False) -> np.ndarray:
    """The host's negacyclic transform mod 2^32 - 2^20 + 1 (fhe_ring_ntt_host): (count, N) residues -> a new array."""
    out = np.ascontiguousarray(polys, dtype=np.uint32).copy()
    out = out.reshape(-1, out.shape[-1])
    _check(lib().fhe_ring_ntt_host(out.shape[1], int(bool(inverse)), _ptr(out), out.shape[0]))
    return out


def ring_product_host(a, b) -> np.ndarray:
    """sum over the terms of a[t] (*) b[t], negacyclic, for (terms, N) signed 32-bit coefficients, through the transform
    (fhe_ring_product_host): N int64, exact while the true magnitude stays below P / 2."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    out = np.zeros(a.shape[1], dtype=np.int64)
    _check(lib().fhe_ring_product_host(a.shape[1], a.shape[0], _ptr(a), _ptr(b), _ptr(out)))
    return out


def packed_glwe_len(params: Params, count: int) -> int:
    return int(lib().fhe_packed_glwe_len(C.byref(params.c()), count))


def packing_keyswitch_host(params: Params, pp, pksk, cts) -> np.ndarray:
    """The packing keyswitch as a plain CPU loop (fhe_packing_keyswitch_host): cts (count, kN+1) ->
    (ceil(count / N), k+1, N).  Bit-identical to Engine.pack."""
    cts = _u64(cts).reshape(-1, params.big_size)
    pksk = _u64(pksk).reshape(-1)
    if pksk.size != packing_key_len(params, pp) or not pksk.size:
        raise FheError(_last_error() if not packing_key_len(params, pp) else "packing key: size does not match the parameter set")
    out = np.zeros((-(-cts.shape[0] // params.N), params.k + 1, params.N), dtype=np.uint64)
    _check(lib().fhe_packing_keyswitch_host(C.byref(params.c()), C.byref(_pp(pp)), _ptr(pksk), _ptr(cts), cts.shape[0], _ptr(out)))
    return out


def glwe_sample_extract_host(params: Params, glwes, count: int, first: int = 0) -> np.ndarray:
    """Sample extraction as a plain CPU loop (fhe_glwe_sample_extract_host): blocks first .. first + count - 1 of packed
    GLWEs -> (count, kN+1) big-key LWEs.  Bit-identical to Engine.unpack(..., refresh=False)."""
    glwes = _u64(glwes).reshape(-1)
    glwe_len = (params.k + 1) * params.N
    if glwes.size % glwe_len or (first + count + params.N - 1) // params.N * glwe_len > glwes.size:
        raise FheError(f"glwe_sample_extract_host: {glwes.size} words do not hold packed block {first + count - 1} of this parameter set")
    out = np.zeros((count, params.big_size), dtype=np.uint64)
    _check(lib().fhe_glwe_sample_extract_host(C.byref(params.c()), _ptr(glwes), first, count, _ptr(out)))
    return out


def packing_unpack_noise(params: Params, pp) -> tuple:
    """(variance of a raw block extracted from a packed PBS output, in nominal units; the default PBS-input budget):
    fhe_packing_unpack_noise.  Engine.unpack(refresh=True) is refused where the first exceeds the second."""
    return tuple(_record(C.c_double, 2, lib().fhe_packing_unpack_noise, C.byref(params.c()), C.byref(_pp(pp))))


class PackedString(np.ndarray):
    """Packed results as a value that goes back in: the GLWE words (n_glwe, k+1, N) as Engine.pack returns them -- it IS
    that array, ClientKey.decrypt_packed and the wire writers take it unchanged -- with `count`, the blocks it holds
    (block j at coefficient j % N of GLWE j // N), and `capacity`, count // blocks per character.  Every FheStringOps
    method accepts it in place of an expanded operand.  Views (x[0]) keep both attributes."""

    def __new__(cls, glwes, count: int, capacity: int):
        obj = _u64(glwes).view(cls)
        obj.count, obj.capacity = int(count), int(capacity)
        return obj

    def __array_finalize__(self, obj):
        self.count = getattr(obj, "count", 0)
        self.capacity = getattr(obj, "capacity", 0)


def narrow_len(params: Params, held: int, bits: int) -> int:
    """u64 words of the narrow list of `held` packed blocks at `bits` bits (fhe_narrow_len); 0 = refused (bits outside 8 .. 32)."""
    return int(lib().fhe_narrow_len(C.byref(params.c()), held, bits))


def narrow_noise(params: Params, pp, bits: int) -> tuple:
    """(variance of a raw block extracted from a packed PBS output narrowed to `bits`, in nominal units; the default
    PBS-input budget; log2 of the probability that the client decodes such a coefficient wrongly): fhe_narrow_noise."""
    return tuple(_record(C.c_double, 3, lib().fhe_narrow_noise, C.byref(params.c()), C.byref(_pp(pp)), bits))


def narrow_default_bits(params: Params, pp, operand: bool = True) -> int:
    """The smallest width a narrow list may have under the packing pair pp: operand=True, to come back as an operand
    (Engine.unpack_narrow with refresh); operand=False, to be decrypted by the client.  Raises when no width qualifies."""
    bits = C.c_uint32()
    _check(lib().fhe_narrow_default_bits(C.byref(params.c()), C.byref(_pp(pp)), int(bool(operand)), C.byref(bits)))
    return int(bits.value)


def glwe_narrow_host(params: Params, glwes, held: int, bits: int) -> np.ndarray:
    """Narrowing as a plain CPU loop (fhe_glwe_narrow_host): the packed GLWEs of `held` blocks -> narrow_len words.
    Bit-identical to Engine.narrow."""
    glwes = _u64(glwes).reshape(-1)
    if glwes.size != packed_glwe_len(params, held):
        raise FheError(f"glwe_narrow_host: {glwes.size} words are not the packed GLWEs of {held} blocks of this parameter set")
    words = narrow_len(params, held, bits)
    if held and not words:
        raise FheError(f"glwe_narrow_host: a width of {bits} bits is refused (8 .. 32)")
    out = np.zeros(words, dtype=np.uint64)
    _check(lib().fhe_glwe_narrow_host(C.byref(params.c()), _ptr(glwes), held, bits, _ptr(out)))
    return out


def _narrow_words(what, params, narrow, held, bits):
    narrow = _u64(narrow).reshape(-1)
    if narrow.size != narrow_len(params, held, bits) or (held and not narrow.size):
        raise FheError(f"{what}: {narrow.size} words are not the narrow list of {held} blocks at {bits} bits of this parameter set")
    return narrow


def glwe_widen_host(params: Params, narrow, held: int, bits: int) -> np.ndarray:
    """A narrow list back to full GLWEs (fhe_glwe_widen_host): (n_glwe, k+1, N), the body coefficients that hold no block 0."""
    narrow = _narrow_words("glwe_widen_host", params, narrow, held, bits)
    out = np.zeros((-(-held // params.N), params.k + 1, params.N), dtype=np.uint64)
    _check(lib().fhe_glwe_widen_host(C.byref(params.c()), _ptr(narrow), held, bits, _ptr(out)))
    return out


def narrow_sample_extract_host(params: Params, narrow, held: int, bits: int, count: int, first: int = 0) -> np.ndarray:
    """Sample extraction straight from a narrow list as a plain CPU loop (fhe_narrow_sample_extract_host): (count, kN+1),
    word for word glwe_sample_extract_host of glwe_widen_host.  Bit-identical to Engine.unpack_narrow(..., refresh=False)."""
    narrow = _narrow_words("narrow_sample_extract_host", params, narrow, held, bits)
    out = np.zeros((count, params.big_size), dtype=np.uint64)
    _check(lib().fhe_narrow_sample_extract_host(C.byref(params.c()), _ptr(narrow), held, bits, first, count, _ptr(out)))
    return out


class NarrowString(np.ndarray):
    """Narrow packed results as a value that goes back in: the words of the narrow list as one row (1, narrow_len) -- so
    that x[0] of a one-output operation keeps the type, like a PackedString's -- with `count`, the blocks it holds,
    `capacity`, count // blocks per character, and `bits`, the width of a coefficient.  ClientKey.decrypt_narrow and
    Engine.unpack_narrow take it as it is; every FheStringOps method accepts it in place of an expanded operand."""

    def __new__(cls, words, count: int, capacity: int, bits: int):
        obj = _u64(words).reshape(1, -1).view(cls)
        obj.count, obj.capacity, obj.bits = int(count), int(capacity), int(bits)
        return obj

    def __array_finalize__(self, obj):
        self.count = getattr(obj, "count", 0)
        self.capacity = getattr(obj, "capacity", 0)
        self.bits = getattr(obj, "bits", 0)


_PACKED = (PackedString, NarrowString)     # the operand forms that go up packed and are unpacked, with refresh, on the device


class Narrow:
    """packed=Narrow(bits): like packed=True, and the packed result is narrowed on the device to `bits`-bit coefficients
    (Engine.narrow); only the narrow words come back, as a NarrowString.  bits=None: the operand-grade default for the
    packing pair given to Engine.load_packing_key, so the result may go straight into the next operation; a result meant
    for the client alone may take narrow_default_bits(params, pp, operand=False)."""
    __slots__ = ("bits",)

    def __init__(self, bits: int | None = None):
        self.bits = None if bits is None else int(bits)

    def __bool__(self):
        return True


def compact_pk_len(params: Params) -> int:
    """Words of a compact public key (2 k N), 0 when k*N is not a power of two (no compact form)."""
    return int(lib().fhe_compact_pk_len(C.byref(params.c())))


def compact_list_len(params: Params, count: int) -> int:
    """Words of a compact list of `count` ciphertexts: ceil(count / kN) * kN + count (0: no compact form)."""
    return int(lib().fhe_compact_list_len(C.byref(params.c()), count))


def compact_conv(lhs, rhs, threads: int = 1) -> np.ndarray:
    """lhs * reverse(rhs) in Z[X]/(X^n + 1), wrapping u64 (slice_semi_reverse_negacyclic_convolution)."""
    lhs, rhs = _u64(lhs).reshape(-1), _u64(rhs).reshape(-1)
    if lhs.size != rhs.size:
        raise FheError("compact_conv: operands of different lengths")
    out = np.zeros(lhs.size, dtype=np.uint64)
    _check(lib().fhe_compact_conv(_ptr(lhs), _ptr(rhs), lhs.size, _ptr(out), threads))
    return out


def expand_compact_host(params: "Params | int", clist, count: int) -> np.ndarray:
    """Host-side expansion of a compact list (fhe_compact_expand_host): (count, kN + 1).  `params` may also be a bare
    power-of-two LWE dimension."""
    dim = params if isinstance(params, int) else params.k * params.N
    clist = _u64(clist).reshape(-1)
    if dim < 2 or dim & (dim - 1):
        raise FheError(f"compact lists need a power-of-two LWE dimension, got {dim}")
    if clist.size != (count + dim - 1) // dim * dim + count:
        raise FheError(f"compact list: {clist.size} words do not hold {count} ciphertexts of dimension {dim}")
    out = np.zeros((count, dim + 1), dtype=np.uint64)
    _check(lib().fhe_compact_expand_host(dim, _ptr(clist), count, _ptr(out)))
    return out


class CompactPublicKey:
    """What a client publishes so that others can encrypt for it (shortint CompactPublicKey, public_key/compact.rs):
    2 k N words, mask then body.  Holds no secret: encrypting takes this key and a seed of the encryptor's own."""

    def __init__(self, params: Params, words):
        self.params = params
        self.words = _u64(words).reshape(-1)
        if self.words.size == 0 or self.words.size != compact_pk_len(params):
            raise FheError("compact public key: size does not match the parameter set")

    def encrypt(self, msgs, seed, threads: int | None = None) -> np.ndarray:
        """Compact list of the messages (each reduced mod msg_mod): compact_list_len(params, len(msgs)) words."""
        msgs = _u64(np.atleast_1d(msgs)).reshape(-1)
        out = np.zeros(compact_list_len(self.params, msgs.size), dtype=np.uint64)
        sb = (C.c_uint8 * 32)(*seed_bytes(seed))
        _check(lib().fhe_compact_pk_encrypt(C.byref(self.params.c()), _ptr(self.words), sb, _ptr(msgs), msgs.size, _ptr(out),
                                            threads or min(16, os.cpu_count() or 1)))
        return out

    def encrypt_string(self, s: bytes, cap: int, seed, threads: int | None = None) -> np.ndarray:
        """Compact list of the cap * blocks_per_char blocks of a zero padded string (string_to_blocks)."""
        return self.encrypt(string_to_blocks(self.params, s, cap), seed, threads)


class Plan(_Handle):
    """A levelised shortint circuit (include/fhestr.h, "plans").  Build with input/lut/lin/pbs/output
    + finalize, or get a ready-made FheString operation from Plan.string_op."""
    _destroy = "fhe_plan_destroy"

    def __init__(self, engine: "Engine | None", handle=None, params: Params | None = None):
        """engine=None builds an offline plan (exportable, not runnable) from `params`."""
        self.engine = engine
        self.params = engine.params if engine is not None else params
        self._h = handle or C.c_void_p()
        if handle is None:
            if engine is not None:
                _check(lib().fhe_plan_create(engine.handle, C.byref(self._h)))
            else:
                _check(lib().fhe_plan_create_offline(C.byref(params.c()), C.byref(self._h)))

    @classmethod
    def string_op(cls, engine: "Engine | None", op: str, a_cap: int, b_cap: int = 0,
                  clear: bytes | None = None, world: int = 1, params: Params | None = None) -> "Plan":
        h = C.c_void_p()
        if engine is not None:
            _check(lib().fhe_str_plan_create(engine.handle, op.encode(), a_cap, b_cap, *_clear(clear or b""), world, C.byref(h)))
        else:
            _check(lib().fhe_str_plan_create_offline(C.byref(params.c()), op.encode(), a_cap, b_cap, *_clear(clear or b""),
                                                     world, C.byref(h)))
        return cls(engine, h, params)

    @classmethod
    def integer_op(cls, engine: "Engine | None", op: str, n_blocks: int, scalar: int = 0, world: int = 1,
                   params: Params | None = None) -> "Plan":
        """Radix-integer operation on n_blocks blocks (include/fhestr.h, "radix-integer operations")."""
        h = C.c_void_p()
        if engine is not None:
            _check(lib().fhe_int_plan_create(engine.handle, op.encode(), n_blocks, C.c_uint64(scalar), world, C.byref(h)))
        else:
            _check(lib().fhe_int_plan_create_offline(C.byref(params.c()), op.encode(), n_blocks, C.c_uint64(scalar),
                                                     world, C.byref(h)))
        return cls(engine, h, params)

    def export_luts(self) -> dict:
        """{plan-local LUT id: accumulator}."""
        n = C.c_uint32()
        _check(lib().fhe_plan_lut_count(self._h, C.byref(n)))
        out = {}
        for i in range(n.value):
            acc = np.zeros(self.params.glwe_len, dtype=np.uint64)
            _check(lib().fhe_plan_export_lut(self._h, i, _ptr(acc)))
            out[i] = acc
        return out

    # ---- building ----
    def input(self, degree: int | None = None) -> int:
        node = C.c_uint32()
        d = self.params.msg_mod - 1 if degree is None else degree
        _check(lib().fhe_plan_input(self._h, d, C.byref(node)))
        return node.value

    def lut(self, f) -> int:
        p = self.params
        table = np.array([int(f(i)) for i in range(p.msg_mod * p.carry_mod)], dtype=np.uint64)
        out = C.c_uint32()
        _check(lib().fhe_plan_lut(self._h, _ptr(table), C.byref(out)))
        return out.value

    def lin(self, terms, constant: int = 0) -> int:
        nodes = np.array([t[0] for t in terms] + [0], dtype=np.uint32)
        coeffs = np.array([t[1] for t in terms] + [0], dtype=np.int32)
        out = C.c_uint32()
        _check(lib().fhe_plan_lin(self._h, _ptr(nodes), _ptr(coeffs), len(terms), constant, C.byref(out)))
        return out.value

    def pbs(self, src: int, lut: int, signed: bool = False) -> int:
        """apply_lookup_table; signed=True declares that the input may be negative (padding bit in use)."""
        out = C.c_uint32()
        _check((lib().fhe_plan_pbs_signed if signed else lib().fhe_plan_pbs)(self._h, src, lut, C.byref(out)))
        return out.value

    def pbs_full_box(self, src: int, all: bool) -> int:
        """msg*carry bits reduced in one lookup: (sum == msg*carry) if all else (sum != 0); see include/fhestr.h."""
        out = C.c_uint32()
        _check(lib().fhe_plan_pbs_full_box(self._h, src, int(bool(all)), C.byref(out)))
        return out.value

    def set_owner_hint(self, rank: int):
        """PBS nodes created from now on run on `rank` (-1 = automatic); see include/fhestr.h."""
        _check(lib().fhe_plan_set_owner_hint(self._h, rank))

    def set_noise_budget(self, budget: float):
        _check(lib().fhe_plan_set_noise_budget(self._h, budget))

    def output(self, node: int):
        _check(lib().fhe_plan_output(self._h, node))

    def finalize(self, world: int = 1):
        _check(lib().fhe_plan_finalize(self._h, world))

    # ---- queries ----
    def info(self) -> dict:
        return dict(zip(("n_inputs", "n_outputs", "n_levels", "n_pbs", "pool_slots", "world"),
                        _record(C.c_uint32, 6, lib().fhe_plan_info, self._h)))

    def noise_info(self) -> dict:
        return dict(zip(("max_pbs_input_noise", "budget", "log2_pfail_worst", "gathered_lwes"),
                        _record(C.c_double, 4, lib().fhe_plan_noise_info, self._h)))

    def level_info(self, level: int) -> dict:
        return dict(zip(("jobs", "local_base", "local_size", "e_max", "recv_base", "terms"),
                        _record(C.c_uint32, 8, lib().fhe_plan_level_info, self._h, level)))

    def level_rank_info(self, level: int, rank: int) -> dict:
        return dict(zip(("job_lo", "job_hi", "n_export"), _record(C.c_uint32, 3, lib().fhe_plan_level_rank_info, self._h, level, rank)))

    def export_level(self, level: int) -> dict:
        li = self.level_info(level)
        off = np.zeros(li["jobs"] + 1, dtype=np.uint32)
        src = np.zeros(max(li["terms"], 1), dtype=np.uint32)
        coeff = np.zeros(max(li["terms"], 1), dtype=np.int32)
        cst = np.zeros(max(li["jobs"], 1), dtype=np.uint64)
        n_lut = li["jobs"] if level < self.info()["n_levels"] else 0
        lut = np.zeros(max(n_lut, 1), dtype=np.uint32)
        _check(lib().fhe_plan_export_level(self._h, level, _ptr(off), _ptr(src), _ptr(coeff), _ptr(cst),
                                           _ptr(lut) if n_lut else None))
        return dict(li, off=off, src=src[:li["terms"]], coeff=coeff[:li["terms"]], cst=cst[:li["jobs"]],
                    lut=lut[:n_lut])

    # ---- execution ----
    def run(self, inputs) -> np.ndarray:
        """Single GPU, host buffers."""
        p = self.params
        info = self.info()
        inputs = _u64(inputs).reshape(-1, p.big_size)
        if inputs.shape[0] != info["n_inputs"]:
            raise FheError(f"plan expects {info['n_inputs']} input ciphertexts, got {inputs.shape[0]}")
        out = np.zeros((info["n_outputs"], p.big_size), dtype=np.uint64)
        _check(lib().fhe_plan_run(self._h, _ptr(inputs) if inputs.size else None, _ptr(out)))
        return out

    def run_batch(self, inputs) -> np.ndarray:
        """Many independent instances of the plan in one pass (fhe_plan_run_batch): inputs (instances, n_inputs, kN+1)
        -> outputs (instances, n_outputs, kN+1).  Level l of all instances is one launch."""
        p = self.params
        info = self.info()
        inputs = _u64(inputs)
        if inputs.ndim != 3 or inputs.shape[1:] != (info["n_inputs"], p.big_size):
            raise FheError(f"run_batch expects (instances, {info['n_inputs']}, {p.big_size}) ciphertext words, got {inputs.shape}")
        out = np.zeros((inputs.shape[0], info["n_outputs"], p.big_size), dtype=np.uint64)
        _check(lib().fhe_plan_run_batch(self._h, inputs.shape[0], _ptr(inputs) if inputs.size else None, _ptr(out)))
        return out

    def run_batch_dev(self, d_inputs: int, d_outputs: int, instances: int):
        """The same on device arrays (raw pointers), ordered on the engine's stream; no host synchronisation."""
        _check(lib().fhe_plan_run_batch_dev(self._h, instances, C.c_void_p(d_inputs), C.c_void_p(d_outputs)))

    def run_dev(self, d_inputs: int, d_outputs: int):
        """One instance on device arrays: inputs n_inputs x (kN+1) words as Engine.expand_compact_list(..., d_out=)
        leaves them, outputs n_outputs x (kN+1); ordered on the engine's stream, no host synchronisation."""
        self.run_batch_dev(d_inputs, d_outputs, 1)

    def run_level_rank_dev(self, d_pool: int, level: int, rank: int):
        _check(lib().fhe_plan_run_level_rank_dev(self._h, C.c_void_p(d_pool), level, rank))

    def gather_outputs_dev(self, d_pool: int, d_out: int):
        _check(lib().fhe_plan_gather_outputs_dev(self._h, C.c_void_p(d_pool), C.c_void_p(d_out)))


def int_to_blocks(params: Params, value: int, n_blocks: int) -> np.ndarray:
    """Little-endian radix digits of an unsigned integer (integer/block_decomposition.rs:119-144)."""
    bits = params.msg_mod.bit_length() - 1
    return np.array([(value >> (bits * i)) & (params.msg_mod - 1) for i in range(n_blocks)], dtype=np.uint64)


def blocks_to_int(params: Params, blocks) -> int:
    bits = params.msg_mod.bit_length() - 1
    return sum((int(b) % params.msg_mod) << (bits * i) for i, b in enumerate(np.asarray(blocks).reshape(-1)))


def blocks_per_char(params: Params) -> int:
    return 8 // (params.msg_mod.bit_length() - 1)


def string_to_blocks(params: Params, s: bytes, cap: int) -> np.ndarray:
    """Zero padded, little-endian block digits of every character (integer/block_decomposition.rs:119-144)."""
    if len(s) > cap:
        raise FheError("string longer than its capacity")
    bits = params.msg_mod.bit_length() - 1
    data = np.frombuffer(s.ljust(cap, b"\0"), dtype=np.uint8).astype(np.uint64)
    return np.stack([(data >> (bits * b)) & (params.msg_mod - 1) for b in range(8 // bits)], axis=1).reshape(-1)


def blocks_to_string(params: Params, blocks) -> bytes:
    bits = params.msg_mod.bit_length() - 1
    bpc = 8 // bits
    b = (np.asarray(blocks).reshape(-1, bpc) % params.msg_mod).astype(np.uint64)
    vals = sum(b[:, i] << (bits * i) for i in range(bpc))
    return bytes(int(v) for v in vals).rstrip(b"\0")


def decode_count(params: Params, msgs) -> int:
    """The count of a split result from its decrypted digit blocks (little-endian base msg_mod).  The value max_parts + 1
    says that parts were cut off."""
    return sum((int(d) % params.msg_mod) * params.msg_mod ** i for i, d in enumerate(np.asarray(msgs).reshape(-1)))


def count_input_digits(params: Params, n_max: int) -> int:
    """D: how many base-msg_mod digits an encrypted count with the public bound n_max travels in (the smallest D with
    msg_mod^D > n_max)."""
    if int(n_max) < 1:
        raise FheError("an encrypted count needs a bound n_max >= 1")
    d = 1
    while params.msg_mod ** d <= int(n_max):
        d += 1
    return d


def encode_count(params: Params, n: int, n_max: int) -> np.ndarray:
    """The D clear digits of the count n (little-endian base msg_mod) to encrypt for an operation with the public bound
    n_max.  n may exceed n_max as long as D digits hold it: the operation then acts as for n_max."""
    d = count_input_digits(params, n_max)
    if not 0 <= int(n) < params.msg_mod ** d:
        raise FheError(f"count {n} does not fit the {d} base-{params.msg_mod} digits of n_max = {n_max}")
    return np.array([(int(n) // params.msg_mod ** i) % params.msg_mod for i in range(d)], dtype=np.uint64)


class EncryptedCount:
    """An encrypted count for FheStringOps.repeat / replacen / splitn / rsplitn, or an encrypted position for take / skip /
    split_at / char_at / insert / substring: `digits`, the ciphertexts of its
    little-endian base-msg_mod digits -- fresh encryptions of encode_count(...), or what len, find / rfind (without the
    found block) or a split's count returned, expanded (D, kN+1), a PackedString or a NarrowString -- and the public bound `n_max` that
    travels with them.  n_max=None: the largest value the digits hold, msg_mod^D - 1 (needs `params`)."""
    __slots__ = ("digits", "n_max")

    def __init__(self, digits, n_max: int | None = None, params: Params | None = None):
        self.digits = digits
        if n_max is None:
            if params is None:
                raise FheError("EncryptedCount: give n_max, or params to take the largest value the digits hold")
            d = digits.count if isinstance(digits, _PACKED) else int(np.asarray(digits).shape[0])
            n_max = params.msg_mod ** d - 1
        if int(n_max) < 1:
            raise FheError("an encrypted count needs a bound n_max >= 1")
        self.n_max = int(n_max)


class SplitResult:
    """What the operations that return several strings give back: `count` -- the digit ciphertexts of min(number of
    parts, max_parts + 1) (decode_count); for split_once / rsplit_once the one 0/1 block `found` -- and `parts`, a list
    of max_parts strings of part_cap characters each, left-justified and zero padded (parts that do not exist are all
    zero).  Expanded: arrays (n, kN+1); packed=True: every member is a PackedString of its own, so each part is an
    operand of the next operation."""
    __slots__ = ("count", "parts")

    def __init__(self, count, parts):
        self.count, self.parts = count, list(parts)

    @property
    def found(self):
        return self.count

    def __iter__(self):
        return iter((self.count, self.parts))


# ---- one call, resolved once: the plan name and what goes with it ----
# FheStringOps and StringProgram both describe the operands of a call and ask the resolvers below; neither formats a plan
# name itself.  A string operand is described by its capacity (int), a clear pattern by its bytes, a clear count by an
# int and an encrypted count by NMax(its public bound); None stands for an operand the operation does not take.

class NMax(int):
    """The description of an encrypted count operand: its public bound n_max."""


class StrCall(typing.NamedTuple):
    """A resolved call: the plan `name` with its parameters, `b_cap` (the capacities of the encrypted pattern operands
    together), the `clear` bytes (None: the plan takes none) and `order`: which of the described operands -- by position,
    the string first -- are the plan's inputs, in the plan's order: the string, the encrypted pattern operand(s), then
    the encrypted count, whose digits are the last inputs."""
    name: str
    b_cap: int
    clear: "bytes | None"
    order: tuple


def _is_clear(x) -> bool:
    return isinstance(x, (bytes, bytearray))


def _patterns(what, *pats):
    """The pattern operands of one call, clear or encrypted alike: (name suffix, b_cap, clear bytes, their positions)."""
    pats = [p for p in pats if p is not None]
    clear = [_is_clear(p) for p in pats]
    if not any(clear):
        return "", sum(pats), None, tuple(range(1, 1 + len(pats)))
    if not all(clear):
        raise FheError(f"{what}: `from` and `to` are both clear bytes or both encrypted strings")
    return "_clear", 0, b"".join(map(bytes, pats)), ()


def resolve_binary(op, a_cap, b=None) -> StrCall:
    """The operations on a string and at most one pattern: the comparisons, find / rfind, strip_prefix / strip_suffix,
    concat, matches (b: the pattern text), and with b=None the unary ones."""
    suffix, b_cap, clear, order = _patterns(op, b)
    return StrCall(op + suffix, b_cap, clear, (0,) + order)


def _from_to(what, frm, to, general):
    suffix, b_cap, clear, order = _patterns(what, frm, to)
    if general and clear is None and frm == 0:
        raise FheError(f"{what}: `from` needs a capacity of at least one character")
    return suffix, b_cap, clear, order, len(frm) if clear is not None else frm, len(to) if clear is not None else to


def resolve_replace(a_cap, frm, to, out_cap=None) -> StrCall:
    """out_cap=None: the equal-length in-place form."""
    suffix, b_cap, clear, order, f, t = _from_to("replace", frm, to, out_cap is not None)
    if out_cap is None and f != t:
        raise FheError(f"replace: `from` and `to` of different {'lengths' if suffix else 'capacities'} need an output capacity (out_cap)")
    return StrCall("replace" + suffix + ("" if out_cap is None else f":{f}:{int(out_cap)}"), b_cap, clear, (0,) + order)


def resolve_replacen(a_cap, frm, to, n, out_cap=None) -> StrCall:
    """n: a clear int or NMax(n_max); out_cap=None: the capacity of the string."""
    suffix, b_cap, clear, order, f, _ = _from_to("replacen", frm, to, True)
    counted = isinstance(n, NMax)
    name = f"replacen{'_encn' if counted else ''}{suffix}:{int(n)}:{f}:{int(a_cap if out_cap is None else out_cap)}"
    return StrCall(name, b_cap, clear, (0,) + order + ((3,) if counted else ()))


def resolve_repeat(a_cap, count) -> StrCall:
    """count: a clear int (1..255) or NMax(n_max)."""
    if isinstance(count, NMax):
        return StrCall(f"repeat:{int(count)}", 0, None, (0, 1))
    if not 1 <= int(count) <= 255:
        raise FheError("repeat: count must be in 1..255")
    return StrCall("repeat_clear", 0, bytes([int(count)]), (0,))


def resolve_split(op, a_cap, pat, max_parts, part_cap=None) -> StrCall:
    """The split family; pat=None: split_ascii_whitespace; max_parts: a clear int or NMax(n_max) (splitn / rsplitn)."""
    counted = isinstance(max_parts, NMax)
    if counted and op not in ("splitn", "rsplitn"):
        raise FheError(f"{op}: only splitn and rsplitn take an encrypted count")
    if part_cap is not None and int(part_cap) <= 0:
        raise FheError("split: the part capacity must be > 0")
    suffix, b_cap, clear, order = _patterns(op, pat)
    if order and b_cap == 0:
        raise FheError(f"{op}: the encrypted pattern needs a capacity of at least one character")
    name = (op + ("_encn" if counted else "") + suffix + ("" if op in ("split_once", "rsplit_once") else f":{int(max_parts)}") +
            ("" if part_cap is None else f":{int(part_cap)}"))
    return StrCall(name, b_cap, clear, (0,) + order + ((2,) if counted else ()))


def resolve_slice(op, a_cap, n, t=None, out_cap=None) -> StrCall:
    """take / skip / split_at / char_at / insert; n: a clear int or NMax(n_max); t (insert only): an encrypted string or
    clear bytes; out_cap=None: the capacity of the string, for insert plus that / the length of t."""
    counted = isinstance(n, NMax)
    if (t is not None) != (op == "insert"):
        raise FheError(f"{op}: {'takes the string to insert' if op == 'insert' else 'only insert takes a second string'}")
    if not counted and int(n) < 0:
        raise FheError(f"{op}: the position must be >= 0")
    if out_cap is not None and (op == "char_at" or int(out_cap) <= 0):
        raise FheError(f"{op}: " + ("one character comes back: there is no output capacity" if op == "char_at" else "the output capacity must be > 0"))
    suffix, b_cap, clear, order = _patterns(op, t)
    if order and b_cap == 0:
        raise FheError(f"{op}: the encrypted string to insert needs a capacity of at least one character")
    name = op + ("_encn" if counted else "") + suffix + f":{int(n)}" + ("" if out_cap is None else f":{int(out_cap)}")
    return StrCall(name, b_cap, clear, (0,) + ((2,) if order else ()) + ((1,) if counted else ()))


# ---- combining results: the plan names of the bit logic, select and the count arithmetic (include/fhestr.h) ----
# A call is (plan name, a_cap, b_cap, clear bytes or None, which of the given operands are the plan's inputs, in its order).
COUNT_OPS = ("add", "sub", "eq", "ne", "lt", "le", "gt", "ge")


def resolve_bits(op, k):
    if op not in ("and", "or", "xor", "not") or int(k) < (1 if op == "not" else 2):
        raise FheError(f"{op}: takes at least {1 if op == 'not' else 2} bit(s)")
    return f"{op}:{int(k)}", 0, 0, None, tuple(range(int(k)))


def resolve_select(a, b, out_cap=None):
    """a, b as described for the resolvers above: capacities (b may be clear bytes), or both NMax; the condition is operand 2."""
    if isinstance(a, NMax) or isinstance(b, NMax):
        if not (isinstance(a, NMax) and isinstance(b, NMax)):
            raise FheError("select: both sides are strings (b may be clear bytes) or both are encrypted counts")
        if out_cap is not None:
            raise FheError("select: counts have no output capacity")
        return f"select_count:{int(a)}:{int(b)}", 0, 0, None, (0, 1, 2)
    if _is_clear(a) or not isinstance(a, (int, np.integer)) or not (_is_clear(b) or isinstance(b, (int, np.integer))):
        raise FheError("select: a is an encrypted string, b an encrypted string or clear bytes")
    cap = int(out_cap) if out_cap is not None else max(int(a), len(b) if _is_clear(b) else int(b), 1)
    if cap <= 0:
        raise FheError("select: the output capacity must be > 0")
    if _is_clear(b):
        return f"select_clear:{cap}", int(a), 0, bytes(b), (0, 2)
    return f"select:{cap}", int(a), int(b), None, (0, 1, 2)


def resolve_count(op, a, b):
    """count_<op> on NMax(a_max) and NMax(b_max), or a clear int b (0 .. 2^32 - 1) in as few bytes as hold it."""
    if op not in COUNT_OPS or not isinstance(a, NMax):
        raise FheError(f"count_{op}: the first operand is an encrypted count")
    if isinstance(b, NMax):
        return f"count_{op}:{int(a)}:{int(b)}", 0, 0, None, (0, 1)
    if not isinstance(b, (int, np.integer)) or not 0 <= int(b) < 2 ** 32:
        raise FheError(f"count_{op}: the second operand is an encrypted count or an int in 0 .. 2^32 - 1")
    return f"count_{op}_clear:{int(a)}", 0, 0, int(b).to_bytes(max(1, (int(b).bit_length() + 7) // 8), "little"), (0,)


def count_result_bound(op, a_max, b):
    """The public bound of count_add / count_sub; b: the other bound, or the clear int."""
    return int(a_max) + int(b) if op == "add" else int(a_max)


class FheStringOps:
    """FheString operator surface over one engine (eq/ne/starts_with/ends_with/contains/find/
    to_upper/to_lower, ..., replace / replacen, the split family, take / skip / split_at / char_at / insert at a clear or an
    encrypted position; and what combines their results: bit_and / bit_or / bit_xor / bit_not, select, count_add /
    count_sub / count_eq .. count_ge / count_min / count_max).  Strings are (cap*blocks, kN+1) arrays of big-key LWEs (see string_to_blocks)."""
    _close_rank = 0             # Engine.close: the cached plans go before string programs

    def __init__(self, engine: Engine, out_alloc=None):
        """out_alloc(shape) -> uint64 array the results are written into (default: np.zeros; pass fhestr.pinned_empty --
        or a cache of such buffers -- for large strings: pageable memory moves at a fraction of the PCIe rate).
        An Engine adopts the object (Engine._adopt) and closes its cached plans before it goes itself.  Anything else
        that is passed as `engine` -- resolving a call needs its `params` only, and the CPU tests resolve over such a
        stand-in -- does not: whoever wraps an engine closes the FheStringOps before the engine."""
        self.engine = engine
        self.bpc = blocks_per_char(engine.params)
        self._alloc = out_alloc or (lambda shape: np.zeros(shape, dtype=np.uint64))
        self._plans = {}            # plans of the packed route, destroyed before their engine (Engine.close)
        if isinstance(engine, Engine):
            engine._adopt(self)

    def close(self):
        """Destroy the cached plans of the packed route (Engine.close does it for every FheStringOps over it)."""
        for plan in self._plans.values():
            plan.close()
        self._plans.clear()

    def _plan(self, op, a_cap, b_cap, clear):
        key = (op, a_cap, b_cap, bytes(clear) if clear is not None else None)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = Plan.string_op(self.engine, op, a_cap, b_cap, bytes(clear) if clear is not None else None)
        return plan

    def _on_device(self, what, plan, rows, shared=()):
        """`plan` on device buffers (the device route: see _run), one instance per entry of rows: the instance's operands
        in the plan's input order, expanded arrays or PackedStrings.  shared: the operands that follow, the same for
        every instance.  An expanded operand is uploaded as it is; a PackedString goes up as GLWEs and is unpacked --
        extracted and refreshed -- into its rows on the device (Engine.unpack): its expanded form never crosses PCIe; a
        shared one is unpacked once, into the first instance, and copied to the others on the device.  Returns (the
        output tensor (instances, n_outputs, kN+1), what must stay alive until the engine has been synchronised)."""
        import torch
        big, dev = self.engine.params.big_size, f"cuda:{self.engine.device}"
        info = plan.info()

        def size(x):
            return x.count if isinstance(x, _PACKED) else x.shape[0]

        n_shared = sum(map(size, shared))
        for xs in rows:
            if sum(map(size, xs)) + n_shared != info["n_inputs"]:
                raise FheError(f"{what}: the plan takes {info['n_inputs']} input blocks, got {sum(map(size, xs)) + n_shared}")
        d_in = torch.empty((len(rows), info["n_inputs"], big), dtype=torch.int64, device=dev)
        d_out = torch.empty((len(rows), info["n_outputs"], big), dtype=torch.int64, device=dev)
        flat = d_in.view(-1, big)
        todo = []                                           # (first row, the operand, its words on the device) of the packed operands

        def place(row, x):
            if isinstance(x, _PACKED):
                todo.append((row, x, torch.from_numpy(np.ascontiguousarray(x).view(np.int64).reshape(-1)).to(dev)))
            else:
                flat[row:row + x.shape[0]].copy_(torch.from_numpy(x.view(np.int64)))
            return row + size(x)

        for r, xs in enumerate(rows):
            at = r * info["n_inputs"]
            for x in xs:
                at = place(at, x)
        at, unpacked = info["n_inputs"] - n_shared, []
        for x in shared:
            if isinstance(x, _PACKED):
                unpacked.append((at, size(x)))
                at = place(at, x)
            else:
                d_in[:, at:at + size(x)].copy_(torch.from_numpy(x.view(np.int64)).to(dev))
                at += size(x)
        torch.cuda.synchronize()                            # torch's stream is not ordered with the engine's
        for row, x, d_words in todo:
            if isinstance(x, NarrowString):
                self.engine.unpack_narrow(d_in=d_words.data_ptr(), held=x.count, bits=x.bits, refresh=True, d_out=flat[row].data_ptr())
            else:
                self.engine.unpack(d_in=d_words.data_ptr(), count=x.count, refresh=True, d_out=flat[row].data_ptr())
        if unpacked and len(rows) > 1:
            self.engine.synchronize()
            for lo, n in unpacked:
                d_in[1:, lo:lo + n].copy_(d_in[0, lo:lo + n])
            torch.cuda.synchronize()
        plan.run_batch_dev(d_in.data_ptr(), d_out.data_ptr(), len(rows))
        return d_out, (todo, d_in)

    def _packed_out(self, d_rows, n_blocks, cap, packed):
        """n_blocks result rows on the device, packed where they lie: a PackedString, or with packed=Narrow(...) narrowed
        on the device too, so that only the narrow words cross PCIe: a NarrowString."""
        if not isinstance(packed, Narrow):
            return PackedString(self.engine.pack(d_rows, count=n_blocks), n_blocks, cap)   # synchronises
        import torch
        p, eng = self.engine.params, self.engine
        bits = packed.bits if packed.bits is not None else eng._default_narrow_bits()
        words = narrow_len(p, n_blocks, bits)
        if not words:
            raise FheError(f"Narrow: a width of {bits} bits is refused (8 .. 32)")
        d_glwes = torch.empty((packed_glwe_len(p, n_blocks),), dtype=torch.int64, device=d_rows.device)
        d_narrow = torch.empty((words,), dtype=torch.int64, device=d_rows.device)
        torch.cuda.synchronize()
        eng.pack(d_in=d_rows.data_ptr(), count=n_blocks, d_out=d_glwes.data_ptr())
        eng.narrow(d_in=d_glwes.data_ptr(), held=n_blocks, bits=bits, d_out=d_narrow.data_ptr())
        eng.synchronize()
        return NarrowString(d_narrow.cpu().numpy().view(np.uint64), n_blocks, cap, bits)

    def _finish(self, d_out, n_blocks, packed):
        if packed:
            return self._packed_out(d_out, n_blocks, n_blocks // self.bpc, packed)
        self.engine.synchronize()
        return d_out.cpu().numpy().view(np.uint64)

    def _run_device(self, name, a_cap, b_cap, clear, operands):
        """One instance of the operation's plan on device buffers: (output tensor (n_outputs, kN+1), what must stay alive
        until the engine has been synchronised).  Plans are kept per (plan name, capacities, clear bytes)."""
        d_out, keep = self._on_device(name, self._plan(name, a_cap, b_cap, clear), [operands])
        return d_out[0], keep

    def _run(self, name, a_cap, b_cap, clear, operands, packed=False, digits=None):
        """One resolved call (StrCall): the plan's outputs, (n_outputs, kN+1).  operands: the string and the encrypted
        pattern operand(s); digits: those of an encrypted count, the plan's last inputs.
        The device route, taken with packed=True and whenever an operand is a PackedString: the plan runs on device
        buffers (_on_device).  packed=True: the output goes through the packing keyswitch where it lies
        (Engine.load_packing_key first) and only the GLWEs come back, as a PackedString: (n_glwe, k+1, N), output block j
        at coefficient j % N of GLWE j // N; decrypt with ClientKey.decrypt_packed, or pass it to the next operation.
        Otherwise the output LWEs are downloaded.
        The host route: fhe_str_op on the operands where they lie, each a part of the plan's inputs."""
        if self._dev(packed, *operands, digits):
            d_out, keep = self._run_device(name, a_cap, b_cap, clear, operands + ([digits] if digits is not None else []))
            return self._finish(d_out, d_out.shape[0], packed)
        parts = operands[:1] + [x for x in operands[1:] if x.shape[0]]      # an empty operand (`to` of capacity 0) is no input
        ptrs = (C.c_void_p * len(parts))(*[x.ctypes.data for x in parts])
        caps = (C.c_uint32 * len(parts))(*[x.shape[0] // self.bpc for x in parts])
        args = (self.engine.handle, name.encode(), ptrs, caps, len(parts), _ptr(digits), *_clear(clear))
        n_out = C.c_uint32(0)
        _check(lib().fhe_str_op(*args, None, C.byref(n_out)))               # outputs (builds and caches the plan)
        out = self._alloc((n_out.value, self.engine.params.big_size))
        _check(lib().fhe_str_op(*args, _ptr(out), C.byref(n_out)))
        return out

    def cast(self, string, cast_key: "CastKey", src_cap: int | None = None, pp=None, v_in: float | None = None):
        """A string of the SOURCE client of cast_key -- its block array, a PackedString or a NarrowString as stored --
        as a block array of this engine's client, which every other method takes.  A packed form goes up as it is stored
        and is cast on the GPU (CastKey.cast_packed; a NarrowString is widened there first, CastKey.cast_narrow).  Where
        the destination's blocks hold more message bits, consecutive source blocks are regrouped into one for this call
        (1 -> 2 and 2 -> 4 bits); narrowing a string (to fewer message bits per block) is refused.
        The cast ends in a lookup and is refused when the noise the blocks are DECLARED to carry puts its input above
        the budget (cast_noise).  Block arrays are judged as lookup outputs (1 nominal variance of the source's set).  A
        stored form carries the SOURCE's packing keyswitch on top, and the narrowing's: pass pp, the (base_log, level) the
        source packed with, and the cast is judged at packing_unpack_noise / narrow_noise of the source's set, the figures
        the unpack refresh judges by; a packed form without pp (or v_in) is refused.  v_in overrides either.
        src_cap: the string's capacity in characters, checked when given."""
        if cast_key.engine is not self.engine:
            raise FheError("cast: the casting key is resident on another engine than this FheStringOps' one")
        src, dst = cast_key.cp.src, self.engine.params
        sb, db = src.msg_mod.bit_length() - 1, dst.msg_mod.bit_length() - 1
        if db < sb:
            raise FheError(f"cast: narrowing a string from {sb} to {db} message bits per block is not supported (out of scope: "
                           "it needs the source's server key per block, Engine.cast_prepare)")
        if db % sb:
            raise FheError(f"cast: {sb} message bits per source block do not divide the destination's {db}")
        group, src_bpc = db // sb, 8 // sb
        stored = isinstance(string, _PACKED)
        if not stored:
            string = _u64(string).reshape(-1, src.big_size)
        count = string.count if stored else string.shape[0]
        if count % src_bpc or (src_cap is not None and count != src_cap * src_bpc):
            raise FheError(f"cast: {count} source blocks are not a string of capacity {src_cap if src_cap is not None else count // src_bpc}")
        if v_in is None and stored:
            if pp is None:
                raise FheError("cast: a packed string carries its packing keyswitch's noise: pass pp, the source's packing pair, or v_in")
            v_in = narrow_noise(src, pp, string.bits)[0] if isinstance(string, NarrowString) else packing_unpack_noise(src, pp)[0]
        if isinstance(string, NarrowString):
            return cast_key.cast_narrow(string, mode=CAST_REFRESH, group=group, v_in=v_in)
        if stored:
            return cast_key.cast_packed(string, count, 0, CAST_REFRESH, group=group, v_in=v_in)
        return cast_key.cast(string, CAST_REFRESH, group=group, v_in=v_in)

    def _cap(self, ct):
        if isinstance(ct, _PACKED):
            return ct, ct.count // self.bpc
        ct = _u64(ct).reshape(-1, self.engine.params.big_size)
        return ct, ct.shape[0] // self.bpc

    @staticmethod
    def _dev(packed, *operands):
        """Does this call take the device route?  (packed output asked for, or a packed operand given)"""
        return bool(packed) or any(isinstance(x, _PACKED) for x in operands)

    def _count_operand(self, count: "EncryptedCount"):
        """The digit ciphertexts of an encrypted count, checked against its bound."""
        digits = count.digits
        if not isinstance(digits, _PACKED):
            digits = _u64(digits).reshape(-1, self.engine.params.big_size)
        have = digits.count if isinstance(digits, _PACKED) else digits.shape[0]
        want = count_input_digits(self.engine.params, count.n_max)
        if have != want:
            raise FheError(f"an encrypted count with n_max = {count.n_max} travels in {want} digits, got {have}")
        return digits

    def _describe(self, x):
        """One operand of a call: (what the plan takes of it, its description for the resolvers: see StrCall)."""
        if x is None or _is_clear(x) or isinstance(x, (int, np.integer)):
            return x, x
        if isinstance(x, EncryptedCount):
            return self._count_operand(x), NMax(x.n_max)
        return self._cap(x)

    def _resolved(self, resolve, args, **kw):
        """Resolve a call on `args` (the string first): (the StrCall, a_cap, the string and the encrypted pattern
        operand(s) in the plan's order, the digits of the encrypted count or None)."""
        given, described = zip(*map(self._describe, args))
        call = resolve(*described, **kw)
        operands = [given[i] for i in call.order]
        digits = operands.pop() if isinstance(described[call.order[-1]], NMax) else None
        return call, described[0], operands, digits

    def _call(self, resolve, args, packed, **kw):
        call, a_cap, operands, digits = self._resolved(resolve, args, **kw)
        return self._run(call.name, a_cap, call.b_cap, call.clear, operands, packed, digits)

    def _binary(self, op, a, b, packed=False):
        """b: an encrypted string, clear bytes, or None for the unary operations."""
        return self._call(functools.partial(resolve_binary, op), (a, b), packed)

    def op_many(self, op, rows, b=None, packed=False, count: "EncryptedCount | None" = None):
        """`op` on every row against ONE second operand in a single pass (fhe_str_op_many): rows (count, cap*blocks, kN+1),
        or a sequence of PackedString of one capacity (one per row); b: an encrypted (zero padded) string -- expanded or a
        PackedString --, clear bytes, or None for unary operations.  `op` may be any plan name, parameters included
        ("split:3" -- with clear bytes "split_clear:3" is meant, and may be written).  Returns (count, n_outputs, kN+1); with
        packed=True one PackedString, output o of row r at block r * n_outputs + o.
        count: the encrypted count of an encrypted-count plan name ("repeat:3", "splitn_encn:3", "replacen_encn:2:1:8") or the
        encrypted position of a slice name ("skip_encn:8", "insert_encn:8" with b the string to insert), shared by all rows
        like b; its n_max must be the one in the name."""
        big = self.engine.params.big_size
        digits = self._count_operand(count) if count is not None else None
        clear = b if isinstance(b, (bytes, bytearray)) else None
        enc = None if (b is None or clear is not None) else self._cap(b)
        base, colon, op_params = op.partition(":")          # a parametrised plan name ("split:3", "split_clear:3") keeps its parameters last
        name = base + ("_clear" if clear is not None and not base.endswith("_clear") else "") + colon + op_params
        if isinstance(rows, (list, tuple)) and any(isinstance(r, _PACKED) for r in rows):
            rows = [self._cap(r)[0] for r in rows]
            sizes = {r.count if isinstance(r, _PACKED) else r.shape[0] for r in rows}
            if len(sizes) != 1:
                raise FheError("op_many expects rows of one capacity")
            return self._packed_many(name, rows, sizes.pop() // self.bpc, enc, clear, packed, digits)
        rows = _u64(rows)
        if rows.ndim != 3 or rows.shape[2] != big:
            raise FheError(f"op_many expects rows of shape (count, cap*blocks, {big})")
        n_rows, a_cap = rows.shape[0], rows.shape[1] // self.bpc
        if self._dev(packed, enc[0] if enc else None, digits):
            # every row's outputs after one another: output o of row r is packed block r * n_outputs + o
            return self._packed_many(name, list(rows), a_cap, enc, clear, packed, digits)
        shared = enc[0] if enc else None                    # the pattern operand, then the count's digits
        if digits is not None:
            shared = np.concatenate([shared, digits]) if enc else digits
        args = (self.engine.handle, name.encode(), _ptr(rows), a_cap, n_rows, _ptr(shared), enc[1] if enc else 0, *_clear(clear))
        n_out = C.c_uint32(0)
        _check(lib().fhe_str_op_many(*args, None, C.byref(n_out)))          # outputs per row (builds and caches the plan)
        out = self._alloc((n_rows, n_out.value, big))
        _check(lib().fhe_str_op_many(*args, _ptr(out), C.byref(n_out)))
        return out

    def _packed_many(self, name, rows, a_cap, enc, clear, packed=True, digits=None):
        """The device route of op_many: rows is a list of expanded (cap*blocks, kN+1) arrays or PackedStrings; the shared
        operands (enc: the pattern, digits: an encrypted count) are placed once and copied to every row."""
        shared = ([enc[0]] if enc else []) + ([digits] if digits is not None else [])
        d_out, keep = self._on_device(name, self._plan(name, a_cap, enc[1] if enc else 0, clear), [[r] for r in rows], shared)
        return self._finish(d_out, d_out.shape[0] * d_out.shape[1], packed)

    def eq_many(self, rows, b): return self.op_many("eq", rows, b)[:, 0]
    def ne_many(self, rows, b): return self.op_many("ne", rows, b)[:, 0]
    def contains_many(self, rows, b): return self.op_many("contains", rows, b)[:, 0]
    def starts_with_many(self, rows, b): return self.op_many("starts_with", rows, b)[:, 0]
    def ends_with_many(self, rows, b): return self.op_many("ends_with", rows, b)[:, 0]
    def find_many(self, rows, b): return self.op_many("find", rows, b)
    def matches_many(self, rows, regex): return self.op_many("matches", rows, self._regex(regex))[:, 0]

    def eq(self, a, b, packed=False): return self._binary("eq", a, b, packed)[0]
    def ne(self, a, b, packed=False): return self._binary("ne", a, b, packed)[0]
    def starts_with(self, a, b, packed=False): return self._binary("starts_with", a, b, packed)[0]
    def ends_with(self, a, b, packed=False): return self._binary("ends_with", a, b, packed)[0]
    def contains(self, a, b, packed=False): return self._binary("contains", a, b, packed)[0]
    def find(self, a, b, packed=False): return self._binary("find", a, b, packed)
    def rfind(self, a, b, packed=False): return self._binary("rfind", a, b, packed)
    def eq_ignore_case(self, a, b, packed=False): return self._binary("eq_ignore_case", a, b, packed)[0]
    def lt(self, a, b, packed=False): return self._binary("lt", a, b, packed)[0]
    def le(self, a, b, packed=False): return self._binary("le", a, b, packed)[0]
    def gt(self, a, b, packed=False): return self._binary("gt", a, b, packed)[0]
    def ge(self, a, b, packed=False): return self._binary("ge", a, b, packed)[0]

    @staticmethod
    def _regex(regex):
        return regex.encode() if isinstance(regex, str) else bytes(regex)

    def matches(self, a, regex, packed=False):
        """One 0/1 block: does the clear regular expression match somewhere in the unpadded string?  regex: the pattern
        text of the reference's regex engine, "/^[0-9]+$/", "/ab|cd/i" (grammar and deviations: include/fhestr.h)."""
        return self._binary("matches", a, self._regex(regex), packed)[0]

    def len(self, a, packed=False): return self._binary("len", a, None, packed)
    def is_empty(self, a, packed=False): return self._binary("is_empty", a, None, packed)[0]

    def _strip_affix(self, op, a, pat, packed=False):
        """pat: clear bytes, or an encrypted (zero padded) pattern.  packed=True: ONE packed array, the flag at
        coefficient 0 and the string's blocks after it."""
        out = self._binary(op, a, pat, packed)
        return out if packed else (out[0], out[1:])

    def strip_prefix(self, a, pat, packed=False): return self._strip_affix("strip_prefix", a, pat, packed)
    def strip_suffix(self, a, pat, packed=False): return self._strip_affix("strip_suffix", a, pat, packed)

    def trim_start(self, a, packed=False): return self._binary("trim_start", a, None, packed)
    def trim_end(self, a, packed=False): return self._binary("trim_end", a, None, packed)
    def strip(self, a, packed=False): return self._binary("strip", a, None, packed)
    def to_upper(self, a, packed=False): return self._binary("to_upper", a, None, packed)
    def to_lower(self, a, packed=False): return self._binary("to_lower", a, None, packed)

    def replace(self, a, frm, to, out_cap: int | None = None, packed=False):
        """Replace every leftmost non-overlapping occurrence of frm by to (bytes.replace).  frm / to: both
        clear bytes, or both encrypted strings.  out_cap=None: the equal-length in-place form (encrypted
        operands unpadded).  With out_cap: any lengths, encrypted operands may be zero padded, the result
        has out_cap characters."""
        return self._call(resolve_replace, (a, frm, to), packed, out_cap=out_cap)

    def replacen(self, a, frm, to, n: "int | EncryptedCount", out_cap: int | None = None, packed=False):
        """Replace the first n leftmost non-overlapping occurrences of frm by to (bytes.replace(frm, to, n), Rust's
        str::replacen).  frm / to: both clear bytes, or both encrypted strings (may be zero padded); any lengths; the
        result has out_cap characters (default: the capacity of a) and is cut there.  A clear empty frm is refused.
        n: a clear int, or an EncryptedCount -- then min(n, n_max) occurrences are replaced, n = 0 returns a."""
        return self._call(resolve_replacen, (a, frm, to, n), packed, out_cap=out_cap)

    def _split(self, op, a, pat, max_parts, part_cap=None, packed=False):
        """The split family (include/fhestr.h, fhe_str_split).  pat: clear bytes, an expanded encrypted (zero padded)
        pattern, a PackedString, or None (split_ascii_whitespace).  Returns a SplitResult.  max_parts may be an
        EncryptedCount (splitn / rsplitn only): then its n_max is the number of parts returned."""
        call, a_cap, operands, digits = self._resolved(functools.partial(resolve_split, op), (a, pat, max_parts), part_cap=part_cap)
        once = op in ("split_once", "rsplit_once")
        P = 2 if once else int(max_parts.n_max if digits is not None else max_parts)
        cap = a_cap if part_cap is None else int(part_cap)
        n_part = cap * self.bpc

        if packed:
            # the count blocks and every part packed on their own, where they lie: a part is the next operation's operand
            out, keep = self._run_device(call.name, a_cap, call.b_cap, call.clear, operands + ([digits] if digits is not None else []))
            take = lambda lo, hi, c: self._packed_out(out[lo:hi], hi - lo, c, packed)
        else:
            out = self._run(call.name, a_cap, call.b_cap, call.clear, operands, False, digits)
            take = lambda lo, hi, c: out[lo:hi]
        n_head = out.shape[0] - P * n_part                  # the count's digits; split_once / rsplit_once: the one block `found`
        if n_head < 1:
            raise FheError(f"{call.name}: the plan has {out.shape[0]} outputs, too few for {P} parts of {n_part} blocks")
        head = out[0] if once and not packed else take(0, n_head, 0)
        return SplitResult(head, [take(n_head + p * n_part, n_head + (p + 1) * n_part, cap) for p in range(P)])

    def split(self, a, pat, max_parts, part_cap=None, packed=False): return self._split("split", a, pat, max_parts, part_cap, packed)
    def rsplit(self, a, pat, max_parts, part_cap=None, packed=False): return self._split("rsplit", a, pat, max_parts, part_cap, packed)
    def split_terminator(self, a, pat, max_parts, part_cap=None, packed=False): return self._split("split_terminator", a, pat, max_parts, part_cap, packed)
    def rsplit_terminator(self, a, pat, max_parts, part_cap=None, packed=False): return self._split("rsplit_terminator", a, pat, max_parts, part_cap, packed)
    def split_inclusive(self, a, pat, max_parts, part_cap=None, packed=False): return self._split("split_inclusive", a, pat, max_parts, part_cap, packed)
    def splitn(self, a, pat, n, part_cap=None, packed=False): return self._split("splitn", a, pat, n, part_cap, packed)
    def rsplitn(self, a, pat, n, part_cap=None, packed=False): return self._split("rsplitn", a, pat, n, part_cap, packed)
    def split_once(self, a, pat, part_cap=None, packed=False): return self._split("split_once", a, pat, 2, part_cap, packed)
    def rsplit_once(self, a, pat, part_cap=None, packed=False): return self._split("rsplit_once", a, pat, 2, part_cap, packed)
    def split_ascii_whitespace(self, a, max_parts, part_cap=None, packed=False): return self._split("split_ascii_whitespace", a, None, max_parts, part_cap, packed)

    def concat(self, a, b, packed=False):
        """a ++ b (padding of a removed); b encrypted (any capacity) or clear bytes."""
        return self._binary("concat", a, b, packed)

    def repeat(self, a, count: "int | EncryptedCount", packed=False):
        """a repeated count times.  count: a clear int (1..255), or an EncryptedCount (n_max 1..255): the result then has
        n_max * a_cap characters and holds min(n, n_max) copies -- none for n = 0."""
        return self._call(resolve_repeat, (a, count), packed)

    # ---- slicing at a position: an int, or an EncryptedCount (what find / rfind / len return, or a fresh encryption) ----
    def _slice(self, op, a, n, t=None, out_cap=None, packed=False):
        return self._call(functools.partial(resolve_slice, op), (a, n, t), packed, out_cap=out_cap)

    def take(self, a, n: "int | EncryptedCount", out_cap: int | None = None, packed=False):
        """s[:n] on the unpadded bytes, out_cap characters (default: the capacity of a).  An encrypted n above its bound
        n_max acts as n_max; positions beyond the hidden length clamp as Python's slices do."""
        return self._slice("take", a, n, None, out_cap, packed)

    def truncate(self, a, n, out_cap: int | None = None, packed=False):
        """= take."""
        return self.take(a, n, out_cap, packed)

    def skip(self, a, n: "int | EncryptedCount", out_cap: int | None = None, packed=False):
        """s[n:], left-justified, out_cap characters (default: the capacity of a)."""
        return self._slice("skip", a, n, None, out_cap, packed)

    def substring(self, a, start, length, out_cap: int | None = None, packed=False):
        """s[start:start + length]: take(skip(a, start), length), two plans."""
        rest = self.skip(a, start, None, packed)
        return self.take(rest, length, out_cap, packed)

    def split_at(self, a, n: "int | EncryptedCount", out_cap: int | None = None, packed=False):
        """(s[:n], s[n:]), out_cap characters each; packed=True: each part packed on its own, like split."""
        call, a_cap, operands, digits = self._resolved(functools.partial(resolve_slice, "split_at"), (a, n, None), out_cap=out_cap)
        n_part = (a_cap if out_cap is None else int(out_cap)) * self.bpc
        if packed:
            out, keep = self._run_device(call.name, a_cap, call.b_cap, call.clear, operands + ([digits] if digits is not None else []))
            return tuple(self._packed_out(out[p * n_part:(p + 1) * n_part], n_part, n_part // self.bpc, packed) for p in range(2))
        out = self._run(call.name, a_cap, call.b_cap, call.clear, operands, False, digits)
        return out[:n_part], out[n_part:]

    def char_at(self, a, n: "int | EncryptedCount", packed=False):
        """(the 0/1 block [n < len(s)], the character s[n:n+1] -- zero when the bit is 0).  packed=True: ONE packed array, the
        bit at coefficient 0 and the character's blocks after it."""
        out = self._slice("char_at", a, n, None, None, packed)
        return out if packed else (out[0], out[1:])

    def insert(self, a, n: "int | EncryptedCount", t, out_cap: int | None = None, packed=False):
        """s[:n] + t + s[n:], cut at out_cap characters (default: the capacity of a plus that -- or the length -- of t).
        t: an encrypted (zero padded) string or clear bytes."""
        return self._slice("insert", a, n, t, out_cap, packed)

    # ---- combining results: bits (eq, contains, found, ...), strings and EncryptedCounts (len, find, ...) ----
    def _combine(self, call, given, packed=False):
        """One run of a combining plan name (resolve_bits / resolve_select / resolve_count): the outputs (n_outputs, kN+1),
        or a PackedString.  A bit is one ciphertext row."""
        name, a_cap, b_cap, clear, order = call
        big = self.engine.params.big_size
        operands = [x if isinstance(x, _PACKED) else _u64(x).reshape(-1, big) for x in (given[i] for i in order)]
        kinds = name.split(":")[0]
        for i, x in zip(order, operands):                   # a bit is one block, however it travels (expanded, packed, narrow)
            is_bit = kinds in ("and", "or", "xor", "not") or (kinds.startswith("select") and i == 2)
            have = x.count if isinstance(x, _PACKED) else x.shape[0]
            if is_bit and have != 1:
                raise FheError(f"{name}: operand {i} is a bit, one 0/1 block, got {have} blocks")
        if self._dev(packed, *operands):
            d_out, keep = self._run_device(name, a_cap, b_cap, clear, operands)
            return self._finish(d_out, d_out.shape[0], packed)
        ptrs = (C.c_void_p * len(operands))(*[x.ctypes.data for x in operands])
        counts = (C.c_uint32 * len(operands))(*[x.shape[0] for x in operands])
        args = (self.engine.handle, name.encode(), ptrs, counts, len(operands), *_clear(clear))
        n_out = C.c_uint32(0)
        _check(lib().fhe_str_combine(*args, None, C.byref(n_out)))         # outputs (builds and caches the plan)
        out = self._alloc((n_out.value, big))
        _check(lib().fhe_str_combine(*args, _ptr(out), C.byref(n_out)))
        return out

    def _bits(self, op, bits, packed=False):
        out = self._combine(resolve_bits(op, len(bits)), list(bits), packed)
        return out if packed or op == "not" and len(bits) > 1 else out[0]

    def bit_and(self, *bits, packed=False):
        """AND of two or more 0/1 blocks (what eq, contains, matches, is_empty or the found of find return): one block."""
        return self._bits("and", bits, packed)

    def bit_or(self, *bits, packed=False): return self._bits("or", bits, packed)
    def bit_xor(self, *bits, packed=False): return self._bits("xor", bits, packed)

    def bit_not(self, *bits, packed=False):
        """The negation of every bit given: one block for one bit, (k, kN+1) for k."""
        return self._bits("not", bits, packed)

    def select(self, cond, a, b, out_cap: int | None = None, packed=False):
        """cond ? a : b.  a, b: encrypted strings (expanded, PackedString or NarrowString; b may be clear bytes) -- each side is
        cut or zero padded to out_cap characters (default: the larger capacity) --, or both EncryptedCounts: then an
        EncryptedCount with the larger bound comes back."""
        (ga, da), (gb, db) = self._describe(a), self._describe(b)
        out = self._combine(resolve_select(da, db, out_cap), [ga, gb, cond], packed)
        return EncryptedCount(out, max(da, db)) if isinstance(da, NMax) else out

    def _count(self, op, a: "EncryptedCount", b: "EncryptedCount | int", packed=False):
        if not isinstance(a, EncryptedCount):
            raise FheError(f"count_{op}: the first operand is an EncryptedCount")
        (ga, da), (gb, db) = self._describe(a), self._describe(b)
        out = self._combine(resolve_count(op, da, db), [ga, gb], packed)
        if op in ("add", "sub"):
            return EncryptedCount(out, count_result_bound(op, da, db))
        return out if packed else out[0]

    def count_add(self, a, b, packed=False):
        """a + b of two counts (b: an EncryptedCount or an int): an EncryptedCount with the bound a.n_max + b.n_max (+ b)."""
        return self._count("add", a, b, packed)

    def count_sub(self, a, b, packed=False):
        """max(a - b, 0), Rust's saturating_sub: an EncryptedCount with the bound of a."""
        return self._count("sub", a, b, packed)

    def count_min(self, a, b, packed=False):
        """min(a, b): a comparison and a select (two plans); with an int b: a - max(a - b, 0)."""
        if isinstance(b, EncryptedCount):
            return self.select(self._count("lt", a, b), a, b, packed=packed)
        return self._count("sub", a, self._count("sub", a, b), packed)

    def count_max(self, a, b, packed=False):
        """max(a, b): a comparison and a select (two plans); with an int b: max(a - b, 0) + b."""
        if isinstance(b, EncryptedCount):
            return self.select(self._count("lt", a, b), b, a, packed=packed)
        return self._count("add", self._count("sub", a, b), b, packed)


def _combining_methods(cls):
    """count_eq .. count_ge on FheStringOps and StringProgram alike: thin names over cls._count."""
    for op in COUNT_OPS[2:]:
        def method(self, a, b, _op=op, **kw):
            return self._count(_op, a, b, **kw)
        method.__name__ = f"count_{op}"
        method.__doc__ = f"The bit [a {dict(eq='==', ne='!=', lt='<', le='<=', gt='>', ge='>=')[op]} b] of two counts; b: an encrypted count or an int."
        setattr(cls, f"count_{op}", method)
    return cls


_combining_methods(FheStringOps)


class ProgramValue:
    """A symbolic value of a StringProgram: an input, or a result of one of its operations.  kind: "string" (`cap`
    characters), "bit", or "count" (`n_max`, the public bound its digits travel with); `blocks` ciphertexts; `op`: the
    index of the operation that produced it, None for an input."""
    __slots__ = ("id", "kind", "blocks", "extent", "op")        # (no reference to the program: it is freed when dropped)
    KINDS = ("string", "bit", "count")

    def __init__(self, program, vid: int):
        info = _record(C.c_uint32, 4, lib().fhe_str_program_value_info, program._h, vid)
        self.id = int(vid)
        self.kind, self.blocks, self.extent = self.KINDS[info[0]], info[1], info[2]
        self.op = None if info[3] == 0xFFFFFFFF else info[3]

    @property
    def cap(self):
        if self.kind != "string":
            raise FheError(f"a {self.kind} has no capacity")
        return self.extent

    @property
    def n_max(self):
        if self.kind != "count":
            raise FheError(f"a {self.kind} has no bound n_max")
        return self.extent

    def __repr__(self):
        return f"<{self.kind} {self.extent} ({self.blocks} blocks) of program value {self.id:#x}>"


class ProgramSplit:
    """What a split operation of a StringProgram returns: `count` (split_once / rsplit_once: the bit `found`) and
    `parts`, symbolic strings.  Given to StringProgram.output as a whole it comes back as a SplitResult."""
    __slots__ = ("count", "parts")

    def __init__(self, count, parts):
        self.count, self.parts = count, list(parts)

    @property
    def found(self):
        return self.count

    def __iter__(self):
        return iter((self.count, self.parts))


class StringProgram(_Handle):
    """Several FheString operations recorded into ONE plan (include/fhestr.h, "string programs").  Declare the inputs with
    string(cap) / count(n_max), apply operations -- the methods mirror FheStringOps, operands are symbolic values or clear
    bytes patterns --, declare the results with output(...) and compile().  Independent operations share lookup levels;
    with dedupe (the default) identical sub-circuits are built once.  engine=None: an offline program from `params`."""
    _destroy = "fhe_str_program_destroy"
    _close_rank = 1             # Engine.close: after the string operations' cached plans

    def __init__(self, engine: "Engine | None", params: Params | None = None, dedupe: bool = True):
        self.engine = engine
        self.params = engine.params if engine is not None else params
        self._h = C.c_void_p()
        if engine is not None:
            _check(lib().fhe_str_program_create(engine.handle, C.byref(self._h)))
        else:
            _check(lib().fhe_str_program_create_offline(C.byref(params.c()), C.byref(self._h)))
        if not dedupe:
            _check(lib().fhe_str_program_set_dedupe(self._h, 0))
        self.inputs = []            # ProgramValue, in declaration order
        self.outputs = []           # ProgramValue / ProgramSplit, in output order
        self.n_ops = 0
        if engine is not None:
            engine._adopt(self)

    # ---- declarations ----
    def string(self, cap: int) -> ProgramValue:
        vid = C.c_uint32()
        _check(lib().fhe_str_program_input_string(self._h, cap, C.byref(vid)))
        self.inputs.append(ProgramValue(self, vid.value))
        return self.inputs[-1]

    def count(self, n_max: int) -> ProgramValue:
        vid = C.c_uint32()
        _check(lib().fhe_str_program_input_count(self._h, n_max, C.byref(vid)))
        self.inputs.append(ProgramValue(self, vid.value))
        return self.inputs[-1]

    def bit(self) -> ProgramValue:
        """A bit input: one 0/1 block."""
        vid = C.c_uint32()
        _check(lib().fhe_str_program_input_bit(self._h, C.byref(vid)))
        self.inputs.append(ProgramValue(self, vid.value))
        return self.inputs[-1]

    def op(self, name: str, *operands, clear: bytes | None = None) -> list:
        """A plan name with its parameters ("split_clear:4:8", "replacen_encn:2:4:32", "matches_clear") on symbolic
        operands, in the order the plan takes its inputs: the string, the encrypted pattern operand(s), the count.
        Returns the list of result values (the layout table of include/fhestr.h)."""
        for x in operands:
            if not isinstance(x, ProgramValue):
                raise FheError(f"{name}: operands are values of a StringProgram, got {type(x).__name__}")
        ids = (C.c_uint32 * max(1, len(operands)))(*[x.id for x in operands])
        args = (self._h, name.encode(), ids, len(operands), *_clear(clear or b""))
        res = (C.c_uint32 * 64)()
        n = C.c_uint32()
        rc = lib().fhe_str_program_op(*args, res, 64, C.byref(n))
        if rc and n.value > 64:
            res = (C.c_uint32 * n.value)()
            rc = lib().fhe_str_program_op(*args, res, n.value, C.byref(n))
        _check(rc)
        self.n_ops += 1
        return [ProgramValue(self, res[i]) for i in range(n.value)]

    def _call(self, resolve, *args, **kw):
        """An operation of FheStringOps on symbolic operands, resolved as there: the list of its result values."""
        def describe(x):
            if isinstance(x, ProgramValue):
                return NMax(x.extent) if x.kind == "count" else x.extent      # (a bit where a string belongs: op refuses it)
            if x is None or _is_clear(x) or isinstance(x, (int, np.integer)):
                return x
            raise FheError(f"operands are values of a StringProgram or clear, got {type(x).__name__}")

        call = resolve(*map(describe, args), **kw)
        return self.op(call.name, *[args[i] for i in call.order], clear=call.clear)

    def _binary(self, op, a, b=None):
        return self._call(functools.partial(resolve_binary, op), a, b)

    def eq(self, a, b): return self._binary("eq", a, b)[0]
    def ne(self, a, b): return self._binary("ne", a, b)[0]
    def starts_with(self, a, b): return self._binary("starts_with", a, b)[0]
    def ends_with(self, a, b): return self._binary("ends_with", a, b)[0]
    def contains(self, a, b): return self._binary("contains", a, b)[0]
    def eq_ignore_case(self, a, b): return self._binary("eq_ignore_case", a, b)[0]
    def lt(self, a, b): return self._binary("lt", a, b)[0]
    def le(self, a, b): return self._binary("le", a, b)[0]
    def gt(self, a, b): return self._binary("gt", a, b)[0]
    def ge(self, a, b): return self._binary("ge", a, b)[0]
    def find(self, a, b): return tuple(self._binary("find", a, b))          # (found, index)
    def rfind(self, a, b): return tuple(self._binary("rfind", a, b))
    def matches(self, a, regex): return self._binary("matches", a, FheStringOps._regex(regex))[0]
    def len(self, a): return self._binary("len", a)[0]
    def is_empty(self, a): return self._binary("is_empty", a)[0]
    def to_upper(self, a): return self._binary("to_upper", a)[0]
    def to_lower(self, a): return self._binary("to_lower", a)[0]
    def trim_start(self, a): return self._binary("trim_start", a)[0]
    def trim_end(self, a): return self._binary("trim_end", a)[0]
    def strip(self, a): return self._binary("strip", a)[0]
    def strip_prefix(self, a, pat): return tuple(self._binary("strip_prefix", a, pat))      # (stripped, string)
    def strip_suffix(self, a, pat): return tuple(self._binary("strip_suffix", a, pat))
    def concat(self, a, b): return self._binary("concat", a, b)[0]

    def repeat(self, a, count):
        """count: a clear int (1..255), or a symbolic count: then its n_max copies at most, the capacity n_max * a.cap."""
        return self._call(resolve_repeat, a, count)[0]

    def replace(self, a, frm, to, out_cap: int | None = None):
        """As FheStringOps.replace: frm / to both clear bytes or both symbolic strings; out_cap=None is the equal-length
        in-place form."""
        return self._call(resolve_replace, a, frm, to, out_cap=out_cap)[0]

    def replacen(self, a, frm, to, n, out_cap: int | None = None):
        """As FheStringOps.replacen; n: a clear int or a symbolic count."""
        return self._call(resolve_replacen, a, frm, to, n, out_cap=out_cap)[0]

    def _split(self, op, a, pat, max_parts, part_cap=None):
        res = self._call(functools.partial(resolve_split, op), a, pat, max_parts, part_cap=part_cap)
        return ProgramSplit(res[0], res[1:])

    def split(self, a, pat, max_parts, part_cap=None): return self._split("split", a, pat, max_parts, part_cap)
    def rsplit(self, a, pat, max_parts, part_cap=None): return self._split("rsplit", a, pat, max_parts, part_cap)
    def split_terminator(self, a, pat, max_parts, part_cap=None): return self._split("split_terminator", a, pat, max_parts, part_cap)
    def rsplit_terminator(self, a, pat, max_parts, part_cap=None): return self._split("rsplit_terminator", a, pat, max_parts, part_cap)
    def split_inclusive(self, a, pat, max_parts, part_cap=None): return self._split("split_inclusive", a, pat, max_parts, part_cap)
    def splitn(self, a, pat, n, part_cap=None): return self._split("splitn", a, pat, n, part_cap)
    def rsplitn(self, a, pat, n, part_cap=None): return self._split("rsplitn", a, pat, n, part_cap)
    def split_once(self, a, pat, part_cap=None): return self._split("split_once", a, pat, 2, part_cap)
    def rsplit_once(self, a, pat, part_cap=None): return self._split("rsplit_once", a, pat, 2, part_cap)
    def split_ascii_whitespace(self, a, max_parts, part_cap=None): return self._split("split_ascii_whitespace", a, None, max_parts, part_cap)

    def _slice(self, op, a, n, t=None, out_cap=None):
        return self._call(functools.partial(resolve_slice, op), a, n, t, out_cap=out_cap)

    def take(self, a, n, out_cap: int | None = None): return self._slice("take", a, n, None, out_cap)[0]
    def truncate(self, a, n, out_cap: int | None = None): return self.take(a, n, out_cap)
    def skip(self, a, n, out_cap: int | None = None): return self._slice("skip", a, n, None, out_cap)[0]
    def split_at(self, a, n, out_cap: int | None = None): return tuple(self._slice("split_at", a, n, None, out_cap))
    def char_at(self, a, n): return tuple(self._slice("char_at", a, n))                     # (valid, character)
    def insert(self, a, n, t, out_cap: int | None = None): return self._slice("insert", a, n, t, out_cap)[0]

    def substring(self, a, start, length, out_cap: int | None = None):
        """s[start:start + length]: two operations of this one plan; start / length: clear ints or symbolic counts."""
        return self.take(self.skip(a, start), length, out_cap)

    # ---- combining results, as FheStringOps: bits, strings and counts are symbolic values ----
    @staticmethod
    def _described(x):
        if isinstance(x, ProgramValue):
            return NMax(x.extent) if x.kind == "count" else x.extent if x.kind == "string" else None
        return x

    def _combine(self, call, given):
        name, _, _, clear, order = call
        return self.op(name, *[given[i] for i in order], clear=clear)

    def bit_and(self, *bits): return self._combine(resolve_bits("and", len(bits)), bits)[0]
    def bit_or(self, *bits): return self._combine(resolve_bits("or", len(bits)), bits)[0]
    def bit_xor(self, *bits): return self._combine(resolve_bits("xor", len(bits)), bits)[0]

    def bit_not(self, *bits):
        """Linear inside a program: no lookup is added.  One value for one bit, a tuple for several."""
        res = self._combine(resolve_bits("not", len(bits)), bits)
        return res[0] if len(bits) == 1 else tuple(res)

    def select(self, cond, a, b, out_cap: int | None = None):
        """cond ? a : b on symbolic strings (b may be clear bytes) or on two symbolic counts."""
        return self._combine(resolve_select(self._described(a), self._described(b), out_cap), [a, b, cond])[0]

    def _count(self, op, a, b):
        return self._combine(resolve_count(op, self._described(a), self._described(b)), [a, b])[0]

    def count_add(self, a, b): return self._count("add", a, b)
    def count_sub(self, a, b): return self._count("sub", a, b)

    def count_min(self, a, b):
        """A comparison and a select_count in this one plan; with an int b: a - max(a - b, 0)."""
        if isinstance(b, ProgramValue):
            return self.select(self._count("lt", a, b), a, b)
        return self._count("sub", a, self._count("sub", a, b))

    def count_max(self, a, b):
        if isinstance(b, ProgramValue):
            return self.select(self._count("lt", a, b), b, a)
        return self._count("add", self._count("sub", a, b), b)

    # ---- results ----
    def output(self, *values):
        """The next outputs of the plan: symbolic values, or whole split results."""
        for v in values:
            flat = [v.count] + v.parts if isinstance(v, ProgramSplit) else [v]
            for x in flat:
                if not isinstance(x, ProgramValue):
                    raise FheError(f"output: a value of a StringProgram, got {type(x).__name__}")
                _check(lib().fhe_str_program_output(self._h, x.id))
            self.outputs.append(v)

    def compile(self, world: int = 1) -> "CompiledProgram":
        h = C.c_void_p()
        _check(lib().fhe_str_program_finish(self._h, world, C.byref(h)))
        return CompiledProgram(self, Plan(self.engine, h, self.params))


_combining_methods(StringProgram)


class CompiledProgram:
    """A finished StringProgram: `plan`, an ordinary Plan (inputs = the program's inputs in declaration order, outputs in
    output order), and the call that runs it on operands given as to FheStringOps."""
    _close_rank = 1             # Engine.close: with the string programs

    def __init__(self, program: StringProgram, plan: Plan):
        self.plan, self.engine, self.params = plan, program.engine, program.params
        self.inputs, self.outputs = list(program.inputs), list(program.outputs)
        self.n_inputs = sum(v.blocks for v in self.inputs)
        self._ops = FheStringOps(self.engine) if self.engine is not None else None
        self._info = plan.info()
        if self.engine is not None:
            self.engine._adopt(self)

    def close(self):
        self.plan.close()

    def _operand(self, v, x):
        """The ciphertexts of one operand (expanded array or PackedString), checked against its declaration."""
        if v.kind == "count":
            if not isinstance(x, EncryptedCount):
                raise FheError("a count input takes an EncryptedCount")
            if x.n_max != v.n_max:
                raise FheError(f"the count input was declared with n_max = {v.n_max}, got {x.n_max}")
            x = x.digits
        if not isinstance(x, _PACKED):
            x = _u64(x).reshape(-1, self.params.big_size)
        have = x.count if isinstance(x, _PACKED) else x.shape[0]
        if have != v.blocks:
            raise FheError(f"the {v.kind} input of {v.extent} takes {v.blocks} blocks, got {have}")
        return x

    def results_of(self, outputs):
        """The results in output order, cut from the plan's flat outputs (n_outputs, kN+1) -- for a run that went another
        way than __call__ (Plan.run, run_batch_dev, the level / rank calls)."""
        outputs = np.asarray(outputs).reshape(self._info["n_outputs"], -1)
        return self._shape(lambda lo, hi, v: outputs[lo:hi])

    def _shape(self, take):
        """The results in output order; take(lo, hi, value) -> the ciphertexts of output rows [lo, hi)."""
        at = [0]

        def one(v):
            lo = at[0]
            at[0] += v.blocks
            got = take(lo, at[0], v)
            return got[0] if v.kind == "bit" else EncryptedCount(got, v.n_max) if v.kind == "count" else got

        return tuple(SplitResult(one(v.count), [one(p) for p in v.parts]) if isinstance(v, ProgramSplit) else one(v)
                     for v in self.outputs)

    def __call__(self, *operands, packed: bool = False):
        """One run on the device route of FheStringOps: expanded operands are uploaded, PackedString operands are unpacked
        on the device.  Results in output order: a bit as one ciphertext row, a string as (cap*blocks, kN+1), a count as an
        EncryptedCount, a split as a SplitResult; packed=True: every string-valued result (the parts of a split
        included) as a PackedString of its own, ready to be the next operation's operand."""
        if self._ops is None:
            raise FheError("offline program: no engine bound")
        if len(operands) != len(self.inputs):
            raise FheError(f"the program takes {len(self.inputs)} operands, got {len(operands)}")
        d_out, keep = self._ops._on_device("program", self.plan, [[self._operand(v, x) for v, x in zip(self.inputs, operands)]])
        d_out = d_out[0]                                    # (one instance)
        self.engine.synchronize()
        host = None if packed and all(v.kind == "string" for o in self.outputs
                                      for v in ([o.count] + o.parts if isinstance(o, ProgramSplit) else [o])) else d_out.cpu().numpy().view(np.uint64)
        del keep

        def take(lo, hi, v):
            if packed and v.kind == "string":
                return PackedString(self.engine.pack(d_out[lo:hi], count=hi - lo), hi - lo, v.cap)
            return host[lo:hi]

        return self._shape(take)

    def run_many(self, rows, *shared):
        """Many instances in one pass (Plan.run_batch: level l of all instances is one launch).  rows: one sequence of
        expanded operands per instance, the program's first inputs; shared: the remaining inputs, the same for every
        instance.  Returns one result tuple per instance, as __call__ gives them."""
        rows = [list(r) if isinstance(r, (list, tuple)) else [r] for r in rows]
        if not rows:
            return []
        n_row = len(rows[0])
        if any(len(r) != n_row for r in rows) or n_row + len(shared) != len(self.inputs):
            raise FheError(f"run_many: {len(self.inputs)} operands per instance, the rows bring {n_row} and {len(shared)} are shared")
        tail = [self._operand(v, x) for v, x in zip(self.inputs[n_row:], shared)]
        heads = [[self._operand(v, x) for v, x in zip(self.inputs, r)] for r in rows]
        if any(isinstance(x, _PACKED) for xs in heads + [tail] for x in xs):
            raise FheError("run_many takes expanded operands")
        inputs = np.stack([np.concatenate(xs + tail) for xs in heads])
        out = self.plan.run_batch(np.ascontiguousarray(inputs).view(np.uint64))
        return [self._shape(lambda lo, hi, v, i=i: out[i, lo:hi]) for i in range(len(rows))]
