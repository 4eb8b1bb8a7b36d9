/*
 * fhestr.h -- C ABI of the MI355X-native FheString engine (libfhestr.so).
 *
 * Drop-in boundary for the hot path of the reference (tfhe-rs 0.5.0 fork, paths under
 * /root/reference/tfhe/src): the batched shortint `apply_lookup_table` = LWE keyswitch +
 * programmable bootstrap, the LWE linear ops around it, the integer-layer comparison loops that
 * call it, and the FheString operations built from those.  Conventions follow the reference's own
 * C API (c_api/utils.rs:3-28, c_api/shortint/server_key/pbs.rs:24-85): opaque handles, `int`
 * return (0 = ok), results through out-pointers, caller-owned flat u64 buffers.
 *
 * Ciphertext layouts are the reference's (entities/lwe_ciphertext.rs:598-625,
 * lwe_keyswitch_key.rs:77-108, lwe_bootstrap_key.rs, glwe_ciphertext.rs:210-222):
 *   big LWE    [a_0 .. a_{kN-1}, b]          kN+1 u64
 *   small LWE  [a_0 .. a_{n-1}, b]           n+1 u64
 *   KSK        [kN][ks_level (level l first)][n+1] u64
 *   BSK (std)  [n][pbs_level (level 1 first)][k+1 rows][k+1 polys][N] u64
 *   LUT / accumulator  [k+1][N] u64 (mask polynomials zero)
 *
 * Pointers named d_* are device (HBM) pointers on the engine's GPU; all others are host pointers.
 * An engine is bound to one GPU and one HIP stream.  Every entry point that touches an engine (directly or through
 * one of its plans) takes that engine's lock, so several host threads may share one engine the way they share the
 * reference's `Sync` ServerKey (shortint/engine/mod.rs:23-25,184-189 gives each thread its own scratch; here the
 * calls are serialised instead: use one engine per thread or per rank for concurrency).  The asynchronous *_dev calls
 * only enqueue work under the lock: ordering between threads is the callers' business, as with any shared stream.
 */
#ifndef FHESTR_H
#define FHESTR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* shortint/parameters/mod.rs:61-76 (ClassicPBSParameters) and multi_bit.rs (MultiBitPBSParameters);
 * native modulus 2^64, KS->PBS order */
typedef struct fhe_params_t {
    uint32_t n, k, N;
    uint32_t pbs_base_log, pbs_level;
    uint32_t ks_base_log, ks_level;
    uint32_t msg_mod, carry_mod;
    double lwe_std, glwe_std;
    /* 0 or 1: classic PBS.  2: multi-bit PBS with that grouping factor (shortint/parameters/multi_bit.rs,
     * core_crypto/algorithms/lwe_multi_bit_programmable_bootstrapping.rs): the bootstrapping key is then
     * n/g * 2^g GGSWs, standard layout [group][selector][level][row][col][N]. */
    uint32_t grouping_factor;
} fhe_params_t;

typedef struct fhe_engine fhe_engine;

/* Last error message of the calling thread ("" if none). */
const char *fhe_last_error(void);
/* Revision tag of the device kernels in this build (profiles/ counter files are keyed on it). */
const char *fhe_kernel_revision(void);

/* ---- engine + keys ------------------------------------------------------------------------ */
/* replaces ServerKey construction (shortint/engine/server_side.rs:54-160), evaluation side only */
int fhe_engine_create(const fhe_params_t *params, int device, fhe_engine **out);
int fhe_engine_destroy(fhe_engine *eng);
int fhe_engine_params(const fhe_engine *eng, fhe_params_t *out);
/* Upload KSK and standard-domain BSK; the BSK is converted on the GPU to the engine's Fourier
 * layout (replaces par_convert_standard_lwe_bootstrap_key_to_fourier,
 * core_crypto/algorithms/lwe_bootstrap_key_conversion.rs:99-152). */
int fhe_engine_load_keys(fhe_engine *eng, const uint64_t *bsk_std, const uint64_t *ksk);
/* Generate KSK and BSK on the device from the secret keys (k*N and n words, each 0 or 1) and install
 * them: replaces ServerKey::new (shortint/engine/server_side.rs:54-160), i.e.
 * allocate_and_generate_new_lwe_keyswitch_key (core_crypto/algorithms/lwe_keyswitch_key_generation.rs:65-130)
 * and par_allocate_and_generate_new_lwe_bootstrap_key (lwe_bootstrap_key_generation.rs:237-300), followed by
 * the Fourier conversion.  Same randomness as fhe_client_gen_server_keys: for one (secret keys, seed)
 * the keys are bit-identical.  bsk_std_out / ksk_out (either may be NULL) receive the standard-domain
 * keys (fhe_params_{bsk,ksk}_len words). */
int fhe_engine_generate_keys(fhe_engine *eng, const uint64_t *glwe_sk, const uint64_t *small_sk,
                             const uint8_t seed[32], uint64_t *bsk_std_out, uint64_t *ksk_out);
/* The engine's HIP stream (hipStream_t) so callers can order their own work against it. */
void *fhe_engine_stream(fhe_engine *eng);
/* Launch on a caller-owned hipStream_t instead (NULL = HIP's default stream), e.g. the framework
 * stream RCCL collectives are enqueued on, so no host synchronisation is needed between a level's
 * kernels and its all-gather.  fhe_engine_reset_stream goes back to the engine's own stream. */
int fhe_engine_set_stream(fhe_engine *eng, void *hip_stream);
int fhe_engine_reset_stream(fhe_engine *eng);
int fhe_engine_synchronize(fhe_engine *eng);
/* Choose the blind-rotation variant: points per thread = 2^log2_points (0 = automatic). */
int fhe_engine_set_variant(fhe_engine *eng, int log2_points);
/* Throughput mode for back-to-back fhe_ks_pbs_batch_dev calls on the engine's own stream (off by default): the
 * keyswitch of call k+1 runs on a second stream, in a 64-register variant whose waves are co-resident with the blind
 * rotation of call k, so it costs (almost) no time of its own: 99.4 k instead of 93.8 k PBS/s on 256-LWE batches of
 * PARAM_MESSAGE_2_CARRY_2.  Results are bit-identical.  Applies to batches of at most one LWE per CU on the
 * register/LDS-resident kernels; other calls run serially as before.
 * ORDERING CONTRACT (differs from the serial mode, where every call is ordered on the engine stream): calls are
 * treated as independent batches.  The engine orders a pipelined call after (a) everything enqueued on the engine
 * stream before the FIRST pipelined call of a run (a run ends with any serial call or synchronisation), (b) an
 * earlier pipelined call whose OUTPUT range overlaps this call's input, (c) the event given through
 * fhe_engine_pipeline_input_event.  Anything else that produces the input -- a kernel or copy the caller enqueued on
 * fhe_engine_stream() between two pipelined calls -- must either be complete on the host or be handed over as such
 * an event; without it the second-stream keyswitch may read the input before it is written.  Outputs are valid
 * after fhe_engine_synchronize.
 * on = 2, "overlapped batches": consecutive calls alternate between two streams and run on the two-LWEs-per-CU kernel, so
 * two batches share the GPU like the two halves of a 512-LWE launch: 256-LWE batches reach the large-batch rate (about
 * 122 k instead of 100 k PBS/s) for the price of each call's latency (4.1 instead of 2.6 ms).  Same ordering contract,
 * plus: a call is also ordered after the previous one if it WRITES what that call reads or writes.  Results are the
 * large-batch kernel's: decrypt-identical to the serial ones and within the same noise, not bit-identical to mode 0 / 1
 * (two f64 transform schedules round differently); bit-identical to serial calls of more than one LWE per CU. */
int fhe_engine_set_pipeline(fhe_engine *eng, int on);
/* One shot: the keyswitch of the NEXT pipelined fhe_ks_pbs_batch_dev call waits for `hip_event` (a hipEvent_t the caller
 * recorded behind the work that produces that call's input, on any stream).  Ignored by serial calls. */
int fhe_engine_pipeline_input_event(fhe_engine *eng, void *hip_event);
/* Multi-bit PBS only: batches of up to max_batch LWEs build every (LWE, group) GGSW on the whole GPU first
 * (prepare_multi_bit_ggsw, lwe_multi_bit_programmable_bootstrapping.rs:18-83, which the reference runs on
 * separate threads) and then rotate against them; larger batches fuse both into one kernel.  Default 64
 * (env FHESTR_MULTIBIT_COMBINE_MAX); 0 = always fused.  Both paths give bit-identical ciphertexts.  Costs
 * max_batch * (n / grouping_factor) * (k+1)^2 * N * 8 bytes of device workspace when used. */
int fhe_engine_set_multibit_combine_max(fhe_engine *eng, uint32_t max_batch);
/* Polynomial sizes N >= 16384 (PARAM_MESSAGE_4_CARRY_4 ...): the blind rotation of one LWE is spread over a
 * cluster of compute units of one XCD that exchange the four-step transform's matrices through that XCD's L2:
 * all 32 CUs of the XCD with two LWEs in flight per XCD for N = 32768 with two levels (round 4), 8 / 4 CUs
 * (N = 32768 / 16384) otherwise.  mode: -1 automatic (default; env FHESTR_CLUSTER), 0 never (one workgroup per
 * LWE through an HBM workspace), 1 always, 2 always and with round 3's 8-CU clusters even where the whole-XCD
 * kernel exists; max_batch: in automatic mode, batches above it take the one-workgroup kernel.  Automatic mode
 * picks the whole-XCD kernel for up to 16 LWEs (one LWE: 12.3 ms against 20.9 ms) and the 8-CU clusters above
 * (four LWEs in flight per XCD: 1.15 k PBS/s at 256 LWEs against 0.85 k).  All kernels read the same Fourier key
 * and give decrypt-identical results. */
int fhe_engine_set_cluster_mode(fhe_engine *eng, int mode, uint32_t max_batch);
/* Latency knob for dependent chains of small batches (the trailing levels of a string comparison): with `on`, a
 * blind-rotation launch that would leave more than half of the compute units idle carries replicas of its workgroups
 * on them (they recompute an LWE of the batch and store nothing).  Results are unchanged; the part keeps drawing power
 * and therefore keeps its clock for the large launch that follows -- otherwise that launch starts 7 % low in shader
 * clock and needs about 14 ms to ramp back (profiles/r03_after_idle.txt).  Costs the energy of the replicas; off by
 * default (FHESTR_KEEP_BUSY=1 turns it on at engine creation).  No counterpart in the reference. */
int fhe_engine_set_keep_busy(fhe_engine *eng, int on);
/* After a synchronisation: clusters the last cluster launch formed (0 if none ran). */
int fhe_engine_cluster_info(fhe_engine *eng, uint32_t *clusters);
/* Which keyswitch kernel the engine's last keyswitch launch ran, as recorded on the host when it was enqueued (no
 * synchronisation; a query, it changes no decision):
 *   info[0]  FHE_KS_KERNEL_NONE before the first launch, else the kernel
 *   info[1]  matrix-core kernel: 32-row tiles per workgroup (1, 2, 4 or 8); byte-plane kernels: samples per workgroup (8, shadow 4)
 *   info[2]  workgroups the sum over the input dimension is split over (grid.z)
 *   info[3]  matrix-core kernel: K steps per such chunk (the last chunk holds info[4] - (info[2] - 1) * info[3]);
 *            byte-plane kernels: input coefficients per chunk
 *   info[4]  matrix-core kernel: K steps in all; byte-plane kernels: the input dimension k * N
 *   info[5]  vector registers per lane of the blind-rotation kernel whose occupancy decides whether throughput mode 1
 *            (fhe_engine_set_pipeline) may run its keyswitch beside it; 0 if the code object does not tell */
#define FHE_KS_KERNEL_NONE 0u
#define FHE_KS_KERNEL_MFMA 1u         /* ks_decompose_kernel + keyswitch_mfma_kernel (int8 matrix cores) */
#define FHE_KS_KERNEL_DOT4 2u         /* keyswitch_dot4_kernel, 8 samples per workgroup (more than 16 levels, FHESTR_KS_MFMA=0) */
#define FHE_KS_KERNEL_DOT4_SHADOW 3u  /* keyswitch_dot4_kernel, 4 samples per workgroup, beside the previous call's blind rotation */
int fhe_engine_keyswitch_info(fhe_engine *eng, uint32_t info[6]);
/* The multi-CU kernels need their whole grid resident at once; when another kernel holds compute units for too long
 * the launch drains with a status instead of hanging, and the engine runs the same batch again on the one-workgroup
 * kernel before the call returns (correct results, that launch's time lost).  count = how often this engine did so. */
int fhe_engine_cluster_fallbacks(fhe_engine *eng, uint32_t *count);

/* ---- lookup tables ------------------------------------------------------------------------- */
/* generate_lookup_table (shortint/server_key/mod.rs:383-399, engine/mod.rs:72-128):
 * table[i] = f(i), i < msg_mod*carry_mod.  Returns the LUT id and its degree (max f). */
int fhe_lut_generate(fhe_engine *eng, const uint64_t *table, uint32_t *lut_id, uint64_t *degree);
/* Upload an already-built accumulator ((k+1)*N u64). */
int fhe_lut_upload(fhe_engine *eng, const uint64_t *accumulator, uint32_t *lut_id);
/* Read an accumulator back ((k+1)*N u64). */
int fhe_lut_download(fhe_engine *eng, uint32_t lut_id, uint64_t *accumulator);
int fhe_lut_count(const fhe_engine *eng, uint32_t *count);

/* ---- the hot path -------------------------------------------------------------------------- */
/* Batch limits of the batched entry points, in one place.  A count above its limit is refused with the message quoted,
 * nothing is launched and the engine stays usable.  Below it, no launch passes a grid dimension above what the device
 * reports (hipDeviceProp_t::maxGridSize, read when the engine is created; an MI355X reports 2147483647 x 65536 x 65536): a
 * grid dimension that grows with the count or with a key size is covered in spans of that size, one launch each
 * (csrc/grid_spans.h).
 *   fhe_keyswitch_batch, fhe_ks_pbs_batch (_dev), fhe_pbs_ks_batch, and every level of fhe_plan_run / fhe_plan_run_batch
 *   (jobs x instances rows of a level are ONE such batch)        524280 LWEs   "batch too large for one keyswitch launch (max 524280 LWEs)"
 *   fhe_pbs_batch                                                2^31 - 1 workgroups of the blind rotation; no check of its own
 *   fhe_engine_pack_lwes (_dev)                                  65535 LWEs    "batch too large for one packing launch (max 65535 LWEs)"
 *   fhe_engine_ring_pack_lwes (_dev)                             65535 LWEs    "batch too large for one ring packing call (max 65535 LWEs)",
 *                                                                and 2 GiB of leaves (count (k+1) N words): refused with the sizes
 *   fhe_cast_lwes, fhe_cast_packed, fhe_cast_narrow (_dev)       65535 blocks  "cast: batch too large for one launch (max 65535 blocks)"
 *   fhe_engine_expand_compact_list (_dev)                        count * ceil(k N / 512) < 2^31 workgroups
 * tests/test_gpu_batch_limits.py runs each of the first, third, fourth and fifth rows at its limit and one past it. */
/* keyswitch_lwe_ciphertext (core_crypto/algorithms/lwe_keyswitch.rs:96-170), batched. */
int fhe_keyswitch_batch(fhe_engine *eng, const uint64_t *lwe_big_in, uint64_t *lwe_small_out,
                        uint32_t count);
/* programmable_bootstrap_lwe_ciphertext_mem_optimized
 * (core_crypto/algorithms/lwe_programmable_bootstrapping.rs:1067-1111), batched; lut_idx may be
 * NULL (LUT 0 for all). */
int fhe_pbs_batch(fhe_engine *eng, const uint64_t *lwe_small_in, const uint32_t *lut_idx,
                  uint64_t *lwe_big_out, uint32_t count);
/* apply_lookup_table / keyswitch_programmable_bootstrap_assign
 * (shortint/server_key/mod.rs:457-476,783-857), batched, host buffers. */
int fhe_ks_pbs_batch(fhe_engine *eng, const uint64_t *lwe_big_in, const uint32_t *lut_idx,
                     uint64_t *lwe_big_out, uint32_t count);
/* Small-key order: programmable_bootstrap_keyswitch_assign (shortint/server_key/mod.rs:859-932, the
 * *_PBS_KS parameter sets): small LWEs in, bootstrap, keyswitch, small LWEs out. */
int fhe_pbs_ks_batch(fhe_engine *eng, const uint64_t *lwe_small_in, const uint32_t *lut_idx,
                     uint64_t *lwe_small_out, uint32_t count);
/* Same with everything resident in HBM; asynchronous on the engine stream. */
int fhe_ks_pbs_batch_dev(fhe_engine *eng, const uint64_t *d_lwe_big_in, const uint32_t *d_lut_idx,
                         uint64_t *d_lwe_big_out, uint32_t count);
/* LWE linear combinations (unchecked_add / scalar_mul / scalar_add / bivariate packing,
 * shortint/server_key/add.rs:520-524, scalar_mul.rs:206-208, scalar_add.rs:211-218,
 * bivariate_pbs.rs:167-182): out[j] = sum_{t in [off[j],off[j+1])} coeff[t]*pool[src[t]],
 * then body += cst[j].  Host buffers. */
int fhe_lwe_lincomb_batch(fhe_engine *eng, const uint64_t *pool, uint32_t pool_count,
                          const uint32_t *off, const uint32_t *src, const int32_t *coeff,
                          const uint64_t *cst, uint64_t *out, uint32_t jobs);
/* Kernel-only timing of the last fhe_ks_pbs_batch*_ call (HIP events on the engine stream):
 * ms[0] = keyswitch, ms[1] = blind rotation + sample extraction. Synchronises. */
int fhe_last_kernel_ms(fhe_engine *eng, float ms[2]);
/* Sum of the kernel durations of the (up to 1024) fhe_ks_pbs_batch* calls recorded since the last
 * reset, measured with HIP events on the engine stream: total_ms[0] keyswitch, total_ms[1] blind
 * rotation; *calls = number of calls summed.  Synchronises; reset != 0 clears the record. */
int fhe_kernel_times(fhe_engine *eng, double total_ms[2], uint32_t *calls, int reset);

/* ---- plans: levelised shortint circuits ----------------------------------------------------- */
/* A plan records shortint operations (LWE linear combinations and apply_lookup_table) as a DAG and
 * executes them level by level, one batched KS+PBS launch per level.  It is the batched replacement
 * of the per-block rayon loops of the reference's integer layer
 * (integer/server_key/radix_parallel/comparison.rs:10-83, scalar_comparison.rs:104-558).
 * With `world` > 1 every PBS has an owner rank; ranks exchange only what another rank consumes (one
 * all-gather per level that exports anything, see fhe_plan_level_info). */
typedef struct fhe_plan fhe_plan;
int fhe_plan_create(fhe_engine *eng, fhe_plan **out);
/* Engine-less plan: can be built, finalised and exported (levels, LUT accumulators) on a host
 * without a GPU -- used by planners and checkers; every run entry point refuses it. */
int fhe_plan_create_offline(const fhe_params_t *params, fhe_plan **out);
int fhe_plan_destroy(fhe_plan *plan);
/* building (before fhe_plan_finalize) */
int fhe_plan_input(fhe_plan *plan, uint64_t degree, uint32_t *node);
int fhe_plan_lut(fhe_plan *plan, const uint64_t *table, uint32_t *lut);    /* generate_lookup_table */
int fhe_plan_lin(fhe_plan *plan, const uint32_t *nodes, const int32_t *coeffs, uint32_t n_terms,
                 int64_t constant, uint32_t *node);                        /* unchecked add/scalar ops */
int fhe_plan_pbs(fhe_plan *plan, uint32_t src, uint32_t lut, uint32_t *node); /* apply_lookup_table */
/* Value ranges are tracked two-sided: fhe_plan_pbs refuses an input that may be negative (it would
 * wrap into the padding bit, shortint/engine/client_side.rs:66-74); fhe_plan_pbs_signed declares that
 * the padding bit is used on purpose and the table is read through its negacyclic extension
 * f(x - msg*carry) = -f(x).  Both refuse inputs above the parameter set's noise budget (in units of one
 * nominal ciphertext variance; MaxNoiseLevel::validate, shortint/ciphertext/mod.rs:28-55). */
int fhe_plan_pbs_signed(fhe_plan *plan, uint32_t src, uint32_t lut, uint32_t *node);
/* Reduction of msg*carry = T bits in one lookup: `src` is a sum with value range [0, T]; the result is the bit
 * (sum == T) if `all`, else (sum != 0).  The reference's are_all_comparisons_block_true /
 * is_at_least_one_comparisons_block_true (integer/server_key/radix_parallel/scalar_comparison.rs:147-233) take T - 1
 * bits per lookup; sum = T is the padding bit, which a table with entries -/+ delta/2 answers consistently (csrc/circuit.h).
 * One level less for AND over a 16-char pattern and OR over up to 256 offsets under PARAM_MESSAGE_2_CARRY_2. */
int fhe_plan_pbs_full_box(fhe_plan *plan, uint32_t src, int all, uint32_t *node);
int fhe_plan_set_noise_budget(fhe_plan *plan, double budget);   /* <= 0: no check */
/* PBS nodes created from now on run on `rank` (-1: automatic).  Used with world > 1 to keep a slice of
 * the work and its first reduction levels on one GPU. */
int fhe_plan_set_owner_hint(fhe_plan *plan, int rank);
int fhe_plan_output(fhe_plan *plan, uint32_t node);
int fhe_plan_finalize(fhe_plan *plan, uint32_t world);
/* info[6] = {n_inputs, n_outputs, n_levels, n_pbs, pool_slots, world} */
int fhe_plan_info(const fhe_plan *plan, uint32_t info[6]);
/* info[4] = {largest PBS-input noise in the plan (nominal variances), the budget, log2 of the modelled
 * failure probability of that worst PBS, ciphertexts a rank receives over all all-gathers} */
int fhe_plan_noise_info(const fhe_plan *plan, double info[4]);
/* out[6] = {V_pbs, V_ks, V_ms (variances, torus = 1), delta/2, default budget, log2 p_fail at it} */
int fhe_noise_model(const fhe_params_t *params, double out[6]);
/* Page-locked host memory (hipHostMalloc).  Every *_host entry point and every FheString call takes plain host
 * pointers; pageable ones move at 3-10 GB/s and page-fault on first touch, buffers from fhe_host_alloc move at the
 * full PCIe rate -- worth it for 1024-char strings under PARAM_MESSAGE_4_CARRY_4 (268 MB each way).  The
 * reference has no counterpart (its ciphertexts are Vec<u64> on the heap, entities/lwe_ciphertext.rs:598-625).
 * fhe_host_free(NULL) is a no-op. */
int fhe_host_alloc(size_t bytes, void **out);
int fhe_host_free(void *ptr);
/* 1 if the model's PBS-output variance has been checked against this engine's measured noise for the shape
 * (N, k, level, grouping factor) of `params`; shapes that have not carry a 4x safety factor in the budget. */
int fhe_noise_model_is_calibrated(const fhe_params_t *params);
/* Would fhe_engine_create accept these parameters?  0 = yes; 1 = no, reason in fhe_last_error.  Needs no device: the
 * same checks fhe_engine_create runs before it touches one (a blind-rotation kernel instantiated for (N, k, level,
 * grouping factor); decomposition ranges of the keyswitch -- any level count, more than 16 levels take the byte-plane
 * kernel instead of the matrix-core one).  Covers every ClassicPBSParameters / MultiBitPBSParameters constant of
 * shortint/parameters/{mod,multi_bit,parameters_compact_pk}.rs (tests/test_parameter_tables.py). */
int fhe_params_supported(const fhe_params_t *params);
/* Pool layout of a level.  Every rank runs its own jobs [job_lo, job_hi) of the level (rank_info) and
 * writes job job_lo + i to pool slot local_base + i; if e_max > 0 the level ends with an all-gather of
 * the first e_max slots of every rank's local region into [recv_base, recv_base + world * e_max).
 * info[8] = {jobs, local_base, local_size, e_max, recv_base, n_terms, 0, 0}; level == n_levels describes
 * the output gather (jobs, n_terms only). */
int fhe_plan_level_info(const fhe_plan *plan, uint32_t level, uint32_t info[8]);
/* info[3] = {job_lo, job_hi, n_export} */
int fhe_plan_level_rank_info(const fhe_plan *plan, uint32_t level, uint32_t rank, uint32_t info[3]);
/* CSR description of a level in job order (any pointer may be NULL): off[jobs+1], src/coeff[n_terms]
 * (src = pool slot), cst[jobs] (already scaled by delta), lut[jobs] */
int fhe_plan_export_level(const fhe_plan *plan, uint32_t level, uint32_t *off, uint32_t *src,
                          int32_t *coeff, uint64_t *cst, uint32_t *lut);
/* plan-local LUT ids (the `lut` arrays above) and their accumulators ((k+1)*N u64) */
int fhe_plan_lut_count(const fhe_plan *plan, uint32_t *count);
int fhe_plan_export_lut(const fhe_plan *plan, uint32_t lut, uint64_t *accumulator);
/* single GPU, host buffers: inputs n_inputs x (kN+1), outputs n_outputs x (kN+1) */
int fhe_plan_run(fhe_plan *plan, const uint64_t *inputs, uint64_t *outputs);
/* `instances` independent copies of the plan (finalised for world 1) in ONE pass: level l of all instances is one gather +
 * one keyswitch + one blind-rotation launch over instances x jobs(l) ciphertexts.  This is the reference's throughput shape
 * -- many independent inputs per call (benches/core_crypto/pbs_bench.rs:430-549; rayon over the blocks of an integer,
 * integer/server_key/radix_parallel/comparison.rs:22-28) -- for whole operations: a single FheString::eq pays four dependent
 * single-PBS latencies on a nearly idle GPU (12.8 ms), 32 of them share those four and run at the engine's batch rate.
 * inputs: [instances][n_inputs] ciphertexts, outputs: [instances][n_outputs] (host arrays; _dev: device arrays, ordered on
 * the engine's stream, no host synchronisation).  Every instance's outputs are those of fhe_plan_run on its inputs (the same
 * gathers and tables; batches beyond one LWE per CU run the two-LWEs-per-CU kernel: decrypt-identical, not bit-identical).
 * With several GPUs the instances shard over the ranks -- no collective at all. */
int fhe_plan_run_batch(fhe_plan *plan, uint32_t instances, const uint64_t *inputs, uint64_t *outputs);
int fhe_plan_run_batch_dev(fhe_plan *plan, uint32_t instances, const uint64_t *d_inputs, uint64_t *d_outputs);
/* multi-GPU building blocks (device pool of pool_slots big LWEs; inputs live in slots [0, n_inputs) on
 * every rank): run `rank`'s jobs of one level; gather the outputs once the last level is through. */
int fhe_plan_run_level_rank_dev(fhe_plan *plan, uint64_t *d_pool, uint32_t level, uint32_t rank);
int fhe_plan_gather_outputs_dev(fhe_plan *plan, const uint64_t *d_pool, uint64_t *d_out);

/* ---- radix-integer operations (the reference's integer layer) -------------------------------- */
/* An unsigned radix integer = n_blocks big-key LWE blocks, little endian, log2(msg_mod) bits each
 * (integer/block_decomposition.rs:119-144).  A plan for one operation, run with fhe_plan_run (inputs in
 * the order given) or sharded like any plan:
 *   "add" "sub"                       a, b -> n_blocks blocks (wrapping): unchecked add + parallel one-carry
 *                                     propagation + message_extract (radix_parallel/add.rs:487-624,724-772)
 *   "scalar_add" "scalar_sub"         a, clear `scalar` (radix_parallel/scalar_add.rs:204-222)
 *   "message_extract" "carry_extract" n_blocks blocks with full carries -> their messages / carries
 *   "cmux"                            cond (0/1 block), t, f -> cond ? t : f (radix_parallel/cmux.rs:194-316)
 *   "eq" "ne" "gt" "ge" "lt" "le"     a, b -> one 0/1 block (comparator.rs:193-280, scalar_comparison.rs:147-233)
 *   "scalar_eq" ... "scalar_le"       a, clear `scalar` (at most 64 bits)
 * The scalar is a 64-bit unsigned number, not a number modulo the integer's range.  scalar_add and scalar_sub wrap, so
 * only its low n_blocks * log2(msg_mod) bits matter.  The six scalar comparisons compare with the number itself: a scalar
 * with a bit beyond the integer's is above every value (scalar_comparison.rs:23-60, is_scalar_out_of_bounds), so eq, gt
 * and ge answer 0 and ne, lt and le answer 1 whatever a holds; that plan still takes a's n_blocks inputs and spends one
 * lookup on its constant.  Two encrypted operands are compared two blocks per lookup where the parameter set's noise
 * budget holds the difference of two packed pairs, 2 (1 + msg_mod^2) variances, and block by block where it does not.
 * Blocks of one bit (msg_mod 2) carry a three-valued scan state in base 4: add, sub and their scalar forms on three blocks
 * and more need msg_mod * carry_mod >= 16 and are refused below it. */
int fhe_int_plan_create(fhe_engine *eng, const char *op, uint32_t n_blocks, uint64_t scalar, uint32_t world,
                        fhe_plan **out);
int fhe_int_plan_create_offline(const fhe_params_t *params, const char *op, uint32_t n_blocks, uint64_t scalar,
                                uint32_t world, fhe_plan **out);

/* ---- FheString operations --------------------------------------------------------------------- */
/* An encrypted string = `cap` characters, zero padded, each character 8/log2(msg_mod) big-key LWE
 * blocks, little endian (integer/block_decomposition.rs:119-144): cap * blocks * (kN+1) u64.
 * Results decrypt to what the clear-text function gives on the unpadded ASCII strings.  The zero characters come
 * after the text and nowhere else (the searches with an encrypted pattern rely on it: csrc/str_match.cpp, group_match).
 * op in {"eq","ne","starts_with","ends_with","contains","find"} (+ "_clear" suffix for a clear
 * pattern) or {"to_upper","to_lower","trim_start","trim_end","strip","replace","replace_clear","concat",
 * "concat_clear","repeat_clear","matches_clear"}, or a name of the split family / replacen (see fhe_str_split below) or of an
 * encrypted-count operation (see fhe_str_repeat below).  Outputs: one 0/1 block; find: found block then
 * ceil(log_msg_mod(cap+1)) index digits (little endian); case ops: the whole string. */
int fhe_str_plan_create(fhe_engine *eng, const char *op, uint32_t a_cap, uint32_t b_cap,
                        const uint8_t *clear, uint32_t clear_len, uint32_t world, fhe_plan **out);
int fhe_str_plan_create_offline(const fhe_params_t *params, const char *op, uint32_t a_cap,
                                uint32_t b_cap, const uint8_t *clear, uint32_t clear_len,
                                uint32_t world, fhe_plan **out);
#define FHE_STR_BINARY_DECL(name)                                                                    \
    int fhe_str_##name(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *b,       \
                       uint32_t b_cap, uint64_t *out);                                               \
    int fhe_str_##name##_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap,                  \
                               const uint8_t *pat, uint32_t pat_len, uint64_t *out);
FHE_STR_BINARY_DECL(eq)
FHE_STR_BINARY_DECL(ne)
FHE_STR_BINARY_DECL(starts_with)
FHE_STR_BINARY_DECL(ends_with)
FHE_STR_BINARY_DECL(contains)
FHE_STR_BINARY_DECL(find)
FHE_STR_BINARY_DECL(rfind)            /* last occurrence; same outputs as find */
FHE_STR_BINARY_DECL(eq_ignore_case)   /* ASCII case folding on both sides, then eq */
FHE_STR_BINARY_DECL(lt)               /* lexicographic (byte-wise) order, like Rust's str / Python's bytes */
FHE_STR_BINARY_DECL(le)
FHE_STR_BINARY_DECL(gt)
FHE_STR_BINARY_DECL(ge)
/* concat: a followed by b (a's padding removed); out = (a_cap + b_cap) * blocks LWEs, resp. a_cap + pat_len
 * for the clear form.  Plan op names "concat" / "concat_clear". */
FHE_STR_BINARY_DECL(concat)
/* matches: does the clear regular expression `regex` match somewhere in the unpadded string?  out = one 0/1 block.
 * Plan op name "matches_clear" with the pattern text as the clear operand; fhe_str_op_many takes it too.
 * The pattern text is that of the reference's regex engine (tfhe/examples/regex_engine, `has_match`):
 *   pattern = '/' '^'? regex '$'? '/' 'i'?     '^' and '$' exist only here, outermost, and bind looser than '|':
 *                                              /^ab|cd$/ is ^(ab|cd)$
 *   regex   = term ('|' regex)?                term = factor+
 *   factor  = atom, then at most one of ? * + {n} {n,} {,m} {n,m}
 *   atom    = .  |  \x (the byte x itself)  |  an alphanumeric  |  one of & ; : , ` ~ - _ ! @ # % ' "
 *           |  ( regex )  |  [ class ]         class = ^ class | x-y (alphanumeric ends) | alphanumerics
 * ASCII only; /i ignores ASCII case.  Four deviations from the reference's executor:
 *   1. repeat counts mean what they say (the reference's /^a{,2}$/ accepts "aaa");
 *   2. /i folds class members and range ends as well as literals;
 *   3. //, an empty alternative or group, {} and {n,m} with n > m are refused with a message (the reference panics or
 *      misparses);
 *   4. a character never matches padding: . and [^...] match real characters only, and $ holds at the hidden end (the
 *      position whose next character is zero, or a_cap).
 * The answer equals Python's re.search(b"^?(?:body)\Z?", s, re.DOTALL [| re.I]) on the unpadded bytes, \x read as
 * re.escape(x).  A plain literal builds the existing plan: /abc/ contains_clear, /^abc/ starts_with_clear, /abc$/
 * ends_with_clear, /^abc$/ eq_clear.  Refused when the plan is built, the reason in fhe_last_error: a malformed pattern
 * (with the byte offset), a non-ASCII byte, more than 256 automaton positions after the repeat counts are expanded,
 * a_cap == 0.  It needs msg_mod * carry_mod >= 16. */
int fhe_str_matches_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *regex, uint32_t regex_len,
                          uint64_t *out);
/* Parses a pattern only (no engine): 0, or nonzero with the reason.  *n_positions: character positions of the expanded
 * pattern (the automaton's states); *max_len: the longest match in characters, 0xFFFFFFFF when unbounded.  Both
 * out-pointers are optional. */
int fhe_regex_check(const uint8_t *regex, uint32_t len, uint32_t *n_positions, uint32_t *max_len);
/* repeat: a repeated `count` (clear, 1..255) times; out = count * a_cap * blocks LWEs.  Plan op name
 * "repeat_clear" with the count as the one clear byte. */
int fhe_str_repeat_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint32_t count, uint64_t *out);
/* whitespace = ASCII 9..13 and 32; results are re-padded with zeros (whole string returned) */
int fhe_str_trim_start(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
int fhe_str_trim_end(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
int fhe_str_strip(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
/* replace every leftmost non-overlapping occurrence of `from` by `to` (Rust's str::replace / Python's
 * bytes.replace).
 * Equal-length forms (the string keeps its shape and is rewritten in place): from_to = pat_cap chars of
 * `from` then pat_cap chars of `to`, neither padded.  Plan op names: "replace" (b_cap = 2*pat_cap) /
 * "replace_clear" (clear = from||to).
 * General forms: any lengths, the result has `out_cap` characters (longer results are cut, so give
 * a_cap + max(0, |to| - |from|) * (a_cap / |from|) to be safe).  Encrypted `from` / `to` may be zero
 * padded (hidden lengths; to_cap == 0 deletes); an encrypted `from` that decrypts to the empty string
 * replaces nothing, a clear empty `from` inserts `to` before every character and at the end like Rust and
 * Python do.  Plan op names "replace:<from_cap>:<out_cap>" (b = from || to) and
 * "replace_clear:<from_len>:<out_cap>" (clear = from || to). */
int fhe_str_replace_general(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *from,
                            uint32_t from_cap, const uint64_t *to, uint32_t to_cap, uint32_t out_cap,
                            uint64_t *out);
int fhe_str_replace_clear_general(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *from,
                                  uint32_t from_len, const uint8_t *to, uint32_t to_len, uint32_t out_cap,
                                  uint64_t *out);
int fhe_str_replace(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *from_to,
                    uint32_t pat_cap, uint64_t *out);
int fhe_str_replace_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *from,
                          const uint8_t *to, uint32_t pat_len, uint64_t *out);
/* replacen: replace the first `n` (clear, >= 0) leftmost non-overlapping occurrences (Rust's str::replacen / Python's
 * bytes.replace(from, to, n)); every other argument, the output and the conventions are those of the general replace
 * above (n = 0 returns the string, fitted to out_cap).  A clear empty `from` is refused.  Plan op names
 * "replacen:<n>:<from_cap>:<out_cap>" (b = from || to) and "replacen_clear:<n>:<from_len>:<out_cap>" (clear = from || to). */
int fhe_str_replacen(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *from, uint32_t from_cap,
                     const uint64_t *to, uint32_t to_cap, uint32_t n, uint32_t out_cap, uint64_t *out);
int fhe_str_replacen_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *from, uint32_t from_len,
                           const uint8_t *to, uint32_t to_len, uint32_t n, uint32_t out_cap, uint64_t *out);
/* The operations that return SEVERAL strings.  `op` is one of the names below, without "_clear" and without parameters;
 * the result is Rust's str method of that name, stated here with Python bytes (`sep` non-empty):
 *   "split"                   s.split(sep)
 *   "rsplit"                  s.rsplit(sep)[::-1]       from the right, as Rust yields them; with a self-overlapping
 *                                                       separator the pieces are cut elsewhere than split's
 *   "split_terminator"        split, the last part dropped if it is empty
 *   "rsplit_terminator"       rsplit as above, the first part dropped if it is empty
 *   "split_inclusive"         every part keeps its separator; no empty last part
 *   "splitn" / "rsplitn"      s.split(sep, n - 1) / s.rsplit(sep, n - 1)[::-1]; max_parts IS n (>= 1)
 *   "split_once"              s.partition(sep): (before, after); not found: (s, "")
 *   "rsplit_once"             s.rpartition(sep): (before, after); not found: ("", s)
 *   "split_ascii_whitespace"  s.split(); takes no pattern.  Whitespace = ASCII 9..13 and 32, the set of trim_start /
 *                             trim_end: Rust's is_ascii_whitespace lacks 0x0B (vertical tab), this one has it.
 * The pattern is encrypted (pat, pat_cap characters, may be zero padded: hidden length) or clear (clear, clear_len
 * bytes); give one of them, none for split_ascii_whitespace.  An encrypted pattern that decrypts to the empty string
 * separates nothing -- the convention of replace above, and a deviation from Rust, which splits between all characters.
 * A clear empty pattern is refused when the plan is built (the per-character split is not provided), and so are
 * max_parts == 0 (splitn: n == 0), a part capacity of 0 in a plan name, and a pattern given to split_ascii_whitespace.
 * The number of parts is hidden, so the caller gives max_parts = P (split_once / rsplit_once: ignored, P = 2) and the
 * capacity of every part, part_cap (0 = a_cap).  Outputs, in this order:
 *   1. count = min(number of parts, P + 1) as little-endian base-msg_mod digits, as many as the value P + 1 needs; the
 *      value P + 1 says that parts were cut off.  split_once / rsplit_once: ONE 0/1 block `found` instead.
 *   2. the P parts in the order above, each part_cap characters, left-justified and zero padded (part_cap * blocks
 *      LWEs).  Parts that do not exist are all zero, a part longer than part_cap is cut as replace cuts at out_cap,
 *      parts beyond P are dropped.
 * *n_outputs (optional) = the number of output ciphertexts; with out == NULL the call only builds the plan and returns
 * that number.  Plan op names: "<op>[_clear]:<max_parts>[:<part_cap>]", "split_once[_clear][:<part_cap>]",
 * "rsplit_once[_clear][:<part_cap>]", "split_ascii_whitespace:<max_parts>[:<part_cap>]".  They need msg_mod * carry_mod >= 16. */
int fhe_str_split(fhe_engine *eng, const char *op, const uint64_t *a, uint32_t a_cap, const uint64_t *pat, uint32_t pat_cap,
                  const uint8_t *clear, uint32_t clear_len, uint32_t max_parts, uint32_t part_cap, uint64_t *out,
                  uint32_t *n_outputs);
/* ---- encrypted counts ----
 * repeat, replacen, splitn and rsplitn also take their count n ENCRYPTED.  n arrives as D big-key LWE blocks, its
 * little-endian base-msg_mod digits, each in [0, msg_mod) with nominal noise: fresh encryptions, or the digit outputs of
 * len, find / rfind or a split count.  The caller states a public bound n_max >= 1; D is the smallest number with
 * msg_mod^D > n_max (feeding the D digits of another operation: n_max = msg_mod^D - 1).  A value above the bound acts as
 * the bound: below, n* = min(n, n_max).  In a plan the digits are the LAST inputs: a, the encrypted pattern operand(s) if
 * any, then the D digits.  Everything not said here is as for the clear-count operation above (an empty encrypted
 * pattern selects / separates nothing, results are cut at out_cap / part_cap, the whitespace set).
 *   fhe_str_repeat              a * n*, out = max_count * a_cap * blocks LWEs (n_max = max_count, 1..255); n = 0 gives the
 *                               empty string.  Plan op name "repeat:<n_max>" (a bare "repeat" is refused).
 *   fhe_str_replacen_encn       a.replace(from, to, n*); n = 0 returns a fitted to out_cap.  Plan op names
 *   fhe_str_replacen_encn_clear "replacen_encn:<n_max>:<from_cap>:<out_cap>" (b = from || to) and
 *                               "replacen_encn_clear:<n_max>:<from_len>:<out_cap>" (clear = from || to; an empty clear
 *                               `from` is refused).
 *   fhe_str_splitn_encn         op = "splitn": parts = [] if n* == 0 else a.split(sep, n* - 1); op = "rsplitn":
 *                               parts = [] if n* == 0 else a.rsplit(sep, n* - 1)[::-1].  n_max = max_parts = P.  The
 *                               outputs have exactly the layout of "splitn:<P>" (fhe_str_split): count = len(parts)
 *                               (<= P) in as many digits as the value P + 1 needs, then P parts of part_cap characters
 *                               (0 = a_cap), missing ones all zero.  Pattern arguments, out == NULL and *n_outputs as for
 *                               fhe_str_split.  Plan op names "splitn_encn[_clear]:<P>[:<part_cap>]" and
 *                               "rsplitn_encn[_clear]:<P>[:<part_cap>]"; they need msg_mod * carry_mod >= 16. */
int fhe_str_repeat(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *n_digits, uint32_t max_count,
                   uint64_t *out);
int fhe_str_replacen_encn(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *from, uint32_t from_cap,
                          const uint64_t *to, uint32_t to_cap, const uint64_t *n_digits, uint32_t n_max, uint32_t out_cap,
                          uint64_t *out);
int fhe_str_replacen_encn_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *from, uint32_t from_len,
                                const uint8_t *to, uint32_t to_len, const uint64_t *n_digits, uint32_t n_max,
                                uint32_t out_cap, uint64_t *out);
int fhe_str_splitn_encn(fhe_engine *eng, const char *op, const uint64_t *a, uint32_t a_cap, const uint64_t *pat,
                        uint32_t pat_cap, const uint8_t *clear, uint32_t clear_len, const uint64_t *n_digits,
                        uint32_t max_parts, uint32_t part_cap, uint64_t *out, uint32_t *n_outputs);
/* ---- slicing at a position ----
 * Python slicing on the unpadded bytes s of `a`, at a position n that is clear or ENCRYPTED (n_digits, as the encrypted
 * counts above: D digits with the public bound n_max; a value above the bound acts as the bound, and n_max may exceed
 * a_cap).  Positions beyond the hidden length clamp as Python's slices do; nothing is refused at run time.  `op` is one of:
 *   "take"       s[:n]                       one string of C characters
 *   "skip"       s[n:]                       one string of C characters, left-justified
 *   "split_at"   (s[:n], s[n:])              two strings of C characters each
 *   "char_at"    (n < len(s), s[n:n+1])      one 0/1 block, then one character (blocks LWEs, zero when the bit is 0)
 *   "insert"     s[:n] + t + s[n:]           one string of C characters, cut there; t is encrypted (t, t_cap characters,
 *                                            zero padded: hidden length) or clear (clear, clear_len bytes, may be empty)
 * C = out_cap, the output capacity; 0: a_cap, for insert a_cap + t_cap resp. a_cap + clear_len.  Results are cut or zero
 * padded to C.  char_at takes no output capacity.  n_digits == NULL: n_or_n_max is the clear position n; otherwise it is
 * n_max (>= 1) and n_digits the D digit ciphertexts, the plan's last inputs.  t and clear are read by insert only (give one
 * of them).  *n_outputs and out == NULL as for fhe_str_split.
 * Plan op names: "take:<n>[:<C>]" "skip:<n>[:<C>]" "split_at:<n>[:<C>]" "char_at:<n>" "insert[_clear]:<n>[:<C>]", and with
 * an encrypted position "take_encn:<n_max>[:<C>]" "skip_encn:<n_max>[:<C>]" "split_at_encn:<n_max>[:<C>]"
 * "char_at_encn:<n_max>" "insert_encn[_clear]:<n_max>[:<C>]".  Refused when the plan is built: a missing position, n_max == 0,
 * C == 0, an output capacity on char_at, "_clear" on anything but insert; the _encn names need msg_mod * carry_mod >= 16.
 * substring(s, start, length) is take of skip; truncate is take. */
int fhe_str_slice(fhe_engine *eng, const char *op, const uint64_t *a, uint32_t a_cap, const uint64_t *t, uint32_t t_cap,
                  const uint8_t *clear, uint32_t clear_len, const uint64_t *n_digits, uint32_t n_or_n_max, uint32_t out_cap,
                  uint64_t *out, uint32_t *n_outputs);
/* ---- combining results: bit logic, select, arithmetic on counts ----
 * Every operation above returns a string, a 0/1 bit (eq, contains, matches, is_empty, the `found` of find) or a count (len,
 * find / rfind, the split counts: D digits with a public bound).  The names below combine such results.  Their inputs are
 * listed in plan order; a condition bit always comes last, where the digits of an _encn name come.
 *   "and:<k>" "or:<k>" "xor:<k>"            k bits (k >= 2)                          one bit
 *   "not:<k>"                               k bits (k >= 1)                          k bits, each negated
 *   "select:<C>"                            string a, string b, bit c                string of C characters: c ? a : b, each side
 *                                                                                    cut or zero padded to C
 *   "select_clear:<C>"                      string a, bit c; b = the clear bytes     the same
 *   "select_count:<a_max>:<b_max>"          digits of a, digits of b, bit c          count c ? a : b, bound max(a_max, b_max)
 *   "count_add:<a_max>:<b_max>"             digits of a, digits of b                 count a + b, bound a_max + b_max
 *   "count_sub:<a_max>:<b_max>"                                                      count max(a - b, 0), bound a_max (saturating_sub)
 *   "count_eq" "count_ne" "count_lt" "count_le" "count_gt" "count_ge" ":<a_max>:<b_max>"                 one bit
 *   "<count name>_clear:<a_max>"            digits of a; b = the clear integer: `clear` holds its 1 to 4 little-endian bytes
 *                                           (count_add_clear: bound a_max + b)
 * min and max are a comparison and a select_count.  Result digits are clean -- each in [0, msg_mod - 1], as many as the
 * result's bound needs (the D of the encrypted counts above) -- so a result is the count operand of any _encn name and of
 * the names here as it is; a result bit is 0 or 1 and may be a condition.
 * An operand count above its declared bound: the count_ names apply the clamping of the _encn names -- the value acts as the
 * bound, they compute on min(a, a_max) and min(b, b_max).  select_count passes the chosen digits through as they are: a
 * value above its bound stays above it and acts as the bound in whatever takes the result.
 * fhe_str_plan_create[_offline] build these names with a_cap / b_cap = the capacities of the strings of a select (b_cap = 0
 * for select_clear) and 0 for every other name: a capacity the name does not use must be 0.  Refused when the plan is built,
 * with a message: a missing parameter, k = 0 (k < 2 for and / or / xor), C = 0, a bound of 0, "_clear" on a name without
 * that form (the bit logic, select_count), a clear integer of no bytes or of more than 4, a capacity the name does not
 * use; the count_ names need msg_mod * carry_mod >= 16 (the digit sums of a count do not fit a smaller message-and-carry
 * space).  Every output block of such a plan has gone through a lookup,
 * as for the slices.  The blocks of a select or a select_count are the unchosen side plus one lookup's correction where
 * that fits the box and the budget -- a value in [0, msg_mod - 1] that carries two nominal variances, not one, the
 * tolerance the slices keep for their outputs; every other result block is a single lookup's output.  Inside a string
 * program `not` stays linear and costs no lookup.
 * fhe_str_combine runs one of these names on host buffers: operands[i] = n_blocks[i] ciphertexts, the n_operands operands in
 * plan order (a string: capacity * blocks; a count: its D digits; a bit: 1); the block counts are checked against the name.
 * clear / clear_len: the clear bytes of select_clear, the clear integer of a count name.  out, *n_outputs and out == NULL
 * as for fhe_str_split; the plan is built on the first call and kept in the cache of the one-call operations. */
int fhe_str_combine(fhe_engine *eng, const char *name, const uint64_t *const *operands, const uint32_t *n_blocks,
                    uint32_t n_operands, const uint8_t *clear, uint32_t clear_len, uint64_t *out, uint32_t *n_outputs);
/* ANY FheString operation in one call, by its plan name: the single-row sibling of fhe_str_op_many below, and where every
 * fhe_str_<operation> entry point of this section ends.  Those are shorthands: each one spells a plan name from its
 * arguments (the names are given with them above) and calls this.  `name` is a plan name of fhe_str_plan_create with its
 * parameters ("eq", "find_clear", "replace:2:6", "split_clear:3", "replacen_encn:1:2:6", "matches_clear").  operands: the
 * n_operands (1..3) encrypted strings the plan takes, in its input order -- the string, then the encrypted pattern
 * operand(s): b, or from and to (an empty `to` is left out) --, operands[i] = caps[i] * blocks ciphertexts; they are read
 * where they lie, as parts of the plan's inputs.  n_digits: the D digit ciphertexts of an encrypted count, the plan's last
 * inputs (NULL when the plan takes no encrypted count).  clear / clear_len: the plan's clear bytes (a pattern, from || to,
 * the one byte of repeat_clear, a regular expression), NULL / 0 when it takes none.  out = the plan's outputs (the layout
 * given with the operation above); *n_outputs (optional) = their number; with out == NULL the call only builds the plan
 * and returns that number, as for fhe_str_split.  The plan is built on the first call and kept (the cache of all one-call
 * operations: most recently used first). */
int fhe_str_op(fhe_engine *eng, const char *name, const uint64_t *const *operands, const uint32_t *caps, uint32_t n_operands,
               const uint64_t *n_digits, const uint8_t *clear, uint32_t clear_len, uint64_t *out, uint32_t *n_outputs);
/* Many strings against ONE second operand in one pass (fhe_plan_run_batch on the operation's cached plan): `op` is an
 * operation name of fhe_str_plan_create ("eq", "ne", "contains", "find", "starts_with", "to_lower", ...; "<op>_clear" with
 * a clear pattern), rows = [count][a_cap * blocks] ciphertexts, b = the shared encrypted operand ([b_cap * blocks]
 * ciphertexts, b_cap = 0 and NULL for unary operations and clear patterns), out = [count][n_outputs] ciphertexts,
 * *n_outputs (optional) = outputs per row; with out == NULL the call only builds the plan and returns that number.
 * Plan names with an encrypted count ("repeat:<n_max>", "replacen_encn:...", "splitn_encn:...") share the count as well: b =
 * the pattern operand ([b_cap * blocks] ciphertexts) followed by the D digits, or the digits alone (b_cap = 0) for clear
 * patterns and repeat.  One pattern against 32 rows: FheString::eq 12.8 ms alone, under 5 ms per row. */
int fhe_str_op_many(fhe_engine *eng, const char *op, const uint64_t *rows, uint32_t a_cap, uint32_t count, const uint64_t *b,
                    uint32_t b_cap, const uint8_t *clear, uint32_t clear_len, uint64_t *out, uint32_t *n_outputs);
/* len: ceil(log_msg_mod(cap+1)) little-endian digits; is_empty: one 0/1 block */
int fhe_str_len(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
int fhe_str_is_empty(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
/* strip_prefix / strip_suffix with a clear pattern: out = 1 + cap*blocks LWEs: first a 0/1 block
 * ("the pattern was there and has been removed"), then the resulting string */
int fhe_str_strip_prefix_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *pat,
                               uint32_t pat_len, uint64_t *out);
int fhe_str_strip_suffix_clear(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint8_t *pat,
                               uint32_t pat_len, uint64_t *out);
/* the same with an encrypted, zero padded pattern (hidden length) */
int fhe_str_strip_prefix(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *pat,
                         uint32_t pat_cap, uint64_t *out);
int fhe_str_strip_suffix(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, const uint64_t *pat,
                         uint32_t pat_cap, uint64_t *out);
int fhe_str_to_upper(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);
int fhe_str_to_lower(fhe_engine *eng, const uint64_t *a, uint32_t a_cap, uint64_t *out);

/* ---- string programs: several FheString operations in ONE plan --------------------------------
 * A program records operations by their plan names (fhe_str_plan_create) into one circuit.  The operands of an operation
 * are VALUES: the program's inputs, or results of its earlier operations.  Independent operations share lookup levels (the
 * plan's depth is the maximum of theirs, not the sum), and -- deduplication, on by default -- identical sub-circuits are
 * built once (the four comparisons of one pair cost one comparison and three lookups).  Three kinds of values:
 *   0 string   cap characters, cap * blocks ciphertexts
 *   1 bit      one 0/1 block
 *   2 count    the D little-endian base-msg_mod digits of a number with the public bound n_max (D: the smallest with
 *              msg_mod^D > n_max), as the encrypted-count operations above take it
 * fhe_str_program_op: `op` is a plan name with its parameters; operands are value ids in the order the plan takes its
 * inputs: the string a, the encrypted pattern operand if the name takes one (the replace forms: `from`, then `to` -- leave
 * `to` out to delete), then the count of an encrypted-count name.  A count with fewer digits than the name takes is extended
 * with zero digits, one with more is refused.  Capacities come from the operands.  `clear` is the clear operand of a "_clear"
 * name.  The ids of the results are written to results[0 .. *n_results), cut from the plan's outputs by this table:
 *   eq ne starts_with ends_with contains lt le gt ge eq_ignore_case (+ "_clear"), is_empty, matches_clear    bit
 *   find rfind (+ "_clear")                         bit `found`, count (n_max = a_cap)
 *   len                                             count (n_max = a_cap)
 *   strip_prefix strip_suffix (+ "_clear")          bit `stripped`, string (a_cap)
 *   to_upper to_lower trim_start trim_end strip     string (a_cap)
 *   concat / concat_clear                           string (a_cap + b_cap / a_cap + clear_len)
 *   repeat_clear / repeat:<n_max>                   string (count * a_cap / n_max * a_cap)
 *   replace replace_clear                           string (a_cap)
 *   replace[_clear]:<F>:<C>, replacen[_encn][_clear]:<n>:<F>:<C>      string (C)
 *   split_once rsplit_once [_clear][:<C>]           bit `found`, 2 strings (C, default a_cap)
 *   the other split names [_clear]:<P>[:<C>]        count (n_max = P + 1), P strings (C, default a_cap)
 *   take skip [_encn]:<n>[:<C>]                     string (C, default a_cap)
 *   split_at[_encn]:<n>[:<C>]                       2 strings (C, default a_cap)
 *   char_at[_encn]:<n>                              bit `valid`, string (1)
 *   insert[_encn][_clear]:<n>[:<C>]                 string (C, default a_cap + b_cap / a_cap + clear_len)
 *   and or xor :<k>                                 bit                              operands: k bits
 *   not:<k>                                         k bits                           operands: k bits
 *   select:<C> / select_clear:<C>                   string (C)                       operands: string, string, bit / string, bit
 *   select_count:<a_max>:<b_max>                    count (n_max = max(a_max, b_max))     operands: count, count, bit
 *   count_add:<a_max>:<b_max> / _clear:<a_max>      count (n_max = a_max + b_max / a_max + the integer)   operands: count, count / count
 *   count_sub:<a_max>:<b_max> / _clear:<a_max>      count (n_max = a_max)            operands: count, count / count
 *   count_eq ne lt le gt ge :<a_max>:<b_max> / _clear:<a_max>      bit               operands: count, count / count
 * The names of the last seven rows ("combining results" above) take their operands in the order given, so bits and counts
 * may come first; a wrong kind or number is refused and leaves the program usable.  A bit operand that is the linear result
 * of a `not` is bound as it is: negation costs no lookup inside a program.
 * The _encn names take the position as their count operand: the index of find or a len feeds "skip_encn:<a_cap>" as it is.
 * An operand that is not what a fresh input would be -- a block that is a linear combination, carries more than nominal
 * noise or a wider range than a message -- passes through one cleaning lookup when it is bound; every other operand is
 * bound as it is, at no cost.
 * fhe_str_program_value_info: info = {kind, blocks, capacity or n_max (bit: 1), index of the producing op (0xFFFFFFFF: a
 * program input)}.  fhe_str_program_output declares a value's blocks as the next outputs.  fhe_str_program_finish
 * finalises for `world` ranks and returns an ordinary plan (fhe_plan_run, fhe_plan_run_batch[_dev], the level / rank calls
 * and the export calls take it; destroy it with fhe_plan_destroy): its inputs are the program's inputs in declaration
 * order, its outputs the declared ones in order.  The program itself stays valid for fhe_str_program_value_info until it
 * is destroyed.
 * Refused with a message: a value id of another program or out of range; a wrong kind or number of operands; results_cap
 * too small (*n_results is still set and nothing is built); an op or declaration after finish; finish without outputs; and
 * whatever fhe_str_plan_create refuses for the name, with its message -- after such a refusal the program accepts nothing
 * more, because half an operation may be in its circuit. */
typedef struct fhe_str_program fhe_str_program;
int fhe_str_program_create(fhe_engine *eng, fhe_str_program **out);
int fhe_str_program_create_offline(const fhe_params_t *params, fhe_str_program **out);
int fhe_str_program_destroy(fhe_str_program *prog);
int fhe_str_program_set_dedupe(fhe_str_program *prog, int on);
int fhe_str_program_input_string(fhe_str_program *prog, uint32_t cap, uint32_t *value);
int fhe_str_program_input_count(fhe_str_program *prog, uint32_t n_max, uint32_t *value);
int fhe_str_program_input_bit(fhe_str_program *prog, uint32_t *value);      /* one 0/1 block */
int fhe_str_program_op(fhe_str_program *prog, const char *op, const uint32_t *operands, uint32_t n_operands,
                       const uint8_t *clear, uint32_t clear_len, uint32_t *results, uint32_t results_cap,
                       uint32_t *n_results);
int fhe_str_program_value_info(const fhe_str_program *prog, uint32_t value, uint32_t info[4]);
int fhe_str_program_output(fhe_str_program *prog, uint32_t value);
int fhe_str_program_finish(fhe_str_program *prog, uint32_t world, fhe_plan **out);

/* ---- client side (CPU): keys, encryption, decryption ---------------------------------------- */
/* ClientKey::new / encrypt / decrypt_message_and_carry / ServerKey::new of the reference
 * (shortint/engine/client_side.rs:13-128, shortint/client_key/mod.rs:281-337,
 * shortint/engine/server_side.rs:54-160).
 * Randomness: all of it -- secret keys, masks, noise -- is ChaCha20 keystream under the 256-bit `seed`
 * (one stream per purpose and key row; stands in for the reference's AES-128-CTR concrete-csprng with
 * forked generators).  Published masks are PRF output and reveal neither the seed nor the noise.  Take
 * the seed from fhe_random_seed (the OS CSPRNG) in production; a fixed seed reproduces every key and
 * ciphertext bit for bit and is for tests only.  The seed is as secret as the secret keys. */
typedef struct fhe_client_key fhe_client_key;
int fhe_random_seed(uint8_t seed[32]);
/* the block function itself (known-answer tests): out = ChaCha20(key; words 12,13 = counter, 14,15 = stream) */
int fhe_chacha20_block(const uint8_t key[32], uint64_t counter, uint64_t stream, uint32_t out[16]);
size_t fhe_params_ksk_len(const fhe_params_t *p);
size_t fhe_params_bsk_len(const fhe_params_t *p);
int fhe_client_key_create(const fhe_params_t *params, const uint8_t seed[32], fhe_client_key **out);
int fhe_client_key_destroy(fhe_client_key *ck);
/* msgs[i] in [0, msg_mod*carry_mod); cts: count x (kN+1) u64 (big-key encryption, glwe noise). */
int fhe_client_encrypt(fhe_client_key *ck, const uint64_t *msgs, uint32_t count, uint64_t *cts);
/* message-and-carry decode of every ciphertext. */
int fhe_client_decrypt(fhe_client_key *ck, const uint64_t *cts, uint32_t count, uint64_t *msgs);
/* Standard-domain BSK + KSK for fhe_engine_load_keys (sizes: fhe_params_{bsk,ksk}_len). */
int fhe_client_gen_server_keys(fhe_client_key *ck, uint64_t *bsk_std, uint64_t *ksk, int threads);
/* Copy out the secret keys (either pointer may be NULL): glwe_sk k*N u64, small_sk n u64. */
int fhe_client_secret_keys(fhe_client_key *ck, uint64_t *glwe_sk, uint64_t *small_sk);

/* ---- public-key clients: compact public keys and compact ciphertext lists ------------------------
 * shortint CompactPublicKey / CompactCiphertextList of the reference (M. Joye, eprint 2023/603;
 * shortint/public_key/compact.rs, core_crypto/algorithms/lwe_compact_public_key_generation.rs:15-50,
 * lwe_encryption.rs:1837-1958, lwe_compact_ciphertext_list_expansion.rs:12-58).  n = k*N, the big key's dimension,
 * must be a power of two (compact.rs:65): every k = 1 set and k = 2, N = 1024; the other shapes are refused with a
 * message, where the reference returns None.
 *   public key: 2n words, mask a then body b = conv(a, s) + e          (conv: slice_algorithms.rs:610-659)
 *   list:       one mask of n words per bin of up to n ciphertexts, then one body word per ciphertext:
 *               ceil(count / n) * n + count words (entities/lwe_compact_ciphertext_list.rs:41-63) -- a 256-char
 *               string under PARAM_MESSAGE_2_CARRY_2 is 24.6 KB instead of 16.8 MB of ciphertexts
 *   expansion:  ciphertext i = (mask of bin i / n times X^(n - (i mod n + 1)) in Z[X]/(X^n + 1), body i), a big LWE
 * Messages are reduced mod msg_mod and encoded like fhe_client_encrypt's (compact.rs:25-42); an expanded ciphertext
 * has degree msg_mod - 1 and at most one nominal noise level (compact.rs:181-189): all three noise terms are drawn
 * with glwe_std, the phase error has variance glwe_std^2 (1 + |r|^2 + |s|^2).
 * Randomness as for the client key: ChaCha20 under `seed`, one stream per purpose and bin; one (key, seed, messages)
 * gives one list bit for bit, whatever `threads` is.  Encrypting needs the public key and a seed, no client key.
 * 0 words = the parameter set has no compact form. */
size_t fhe_compact_pk_len(const fhe_params_t *params);
size_t fhe_compact_list_len(const fhe_params_t *params, uint32_t count);
int fhe_client_gen_compact_public_key(fhe_client_key *ck, const uint8_t seed[32], uint64_t *pk_out);
int fhe_compact_pk_encrypt(const fhe_params_t *params, const uint64_t *pk, const uint8_t seed[32], const uint64_t *msgs,
                           uint32_t count, uint64_t *list_out, int threads);
/* Expansion on the host (any power-of-two lwe_dim): out = count x (lwe_dim + 1) words. */
int fhe_compact_expand_host(uint32_t lwe_dim, const uint64_t *list, uint32_t count, uint64_t *out);
/* Expansion on the GPU (csrc/compact_kernels.hip.h): the list goes over PCIe, the ciphertexts are written in HBM, into
 * d_out (device, count x (kN+1) words; may be NULL) and / or host_out -- bit-identical to fhe_compact_expand_host.
 * _dev: the list is already on the device; asynchronous on the engine's stream, no host synchronisation.  d_out is what
 * fhe_ks_pbs_batch_dev and fhe_plan_run_batch_dev read: an expanded ciphertext never has to cross PCIe. */
int fhe_engine_expand_compact_list(fhe_engine *eng, const uint64_t *list, uint32_t count, uint64_t *d_out, uint64_t *host_out);
int fhe_engine_expand_compact_list_dev(fhe_engine *eng, const uint64_t *d_list, uint32_t count, uint64_t *d_out);
/* out = lhs * reverse(rhs) in Z[X]/(X^n + 1), any n >= 1 and any rhs: the convolution behind the three functions above
 * (slice_semi_reverse_negacyclic_convolution; known answer (1, 2, 3), (4, 5, 6) -> (-17, 5, 32)). */
int fhe_compact_conv(const uint64_t *lhs, const uint64_t *rhs, uint32_t n, uint64_t *out, int threads);

/* ---- packing keyswitch: results go back as GLWE ciphertexts ----------------------------------------
 * keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext of the reference
 * (core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187,297-380): up to N big-key LWEs become the coefficients of ONE
 * GLWE ciphertext of (k+1) N words under the client's own GLWE key -- the 1024 result blocks of a 256-character string
 * under PARAM_MESSAGE_2_CARRY_2 are 32 KB instead of 16.8 MB.  For LWE number d of a group,
 *     T_d[p][c]  = [p == k and c == 0] * body_d - sum_{i, lv} digit(a_i, lv) * PKSK[i][lv][p][c]     (mod 2^64)
 *     out[p]    += X^d * T_d[p]                                               in Z[X] / (X^N + 1)
 * with the signed digits of closest_representable(a_i), level L first, as in the LWE keyswitch.  Nothing is rounded:
 * host and GPU give the same words.
 *   key    [kN][level, level L first][k+1][N] u64            (entities/lwe_packing_keyswitch_key.rs)
 *   output ceil(count / N) GLWEs of [k+1][N] u64; LWE j is coefficient j % N of GLWE j / N, unused coefficients
 *          encrypt nothing (0)
 * 1 <= base_log <= 7, level <= 16, base_log * level <= 63; a key above 4 GiB (N >= 16384) is refused and
 * fhe_packing_key_len returns 0. */
typedef struct fhe_packing_params_t {
    uint32_t base_log, level;
} fhe_packing_params_t;
/* Fewest levels, then largest base, for which a packed PBS output decoded at delta / 2 stays within the failure bound
 * a plan enforces at its PBS inputs (csrc/noise_model.h). */
int fhe_packing_default_params(const fhe_params_t *params, fhe_packing_params_t *out);
size_t fhe_packing_key_len(const fhe_params_t *params, const fhe_packing_params_t *pp);   /* words; 0 = refused */
size_t fhe_packed_glwe_len(const fhe_params_t *params, uint32_t count);                   /* words of the output */
/* lwe_packing_keyswitch_key_generation.rs:19-96: for key bit s_i and level l a GLWE encryption of the constant
 * polynomial s_i << (64 - base_log * l) under the GLWE key, noise glwe_std.  ChaCha20 under `seed`, one stream per key
 * bit: the same key whatever `threads` is. */
int fhe_client_gen_packing_key(fhe_client_key *ck, const fhe_packing_params_t *pp, const uint8_t seed[32],
                               uint64_t *pksk_out, int threads);
/* Coefficient j % N of the phase body - sum_q A_q S_q of GLWE j / N, decoded like fhe_client_decrypt. */
int fhe_client_decrypt_packed(fhe_client_key *ck, const uint64_t *glwes, uint32_t count, uint64_t *msgs);
/* The plain loop on the host (parity; callers without a GPU). */
int fhe_packing_keyswitch_host(const fhe_params_t *params, const fhe_packing_params_t *pp, const uint64_t *pksk,
                               const uint64_t *cts, uint32_t count, uint64_t *glwes);
/* Upload the key and rewrite it once into digit planes (csrc/packing_ks_kernels.hip.h); replaces a key loaded before. */
int fhe_engine_load_packing_key(fhe_engine *eng, const fhe_packing_params_t *pp, const uint64_t *pksk);
/* Host ciphertexts in, host GLWEs out; synchronises. */
int fhe_engine_pack_lwes(fhe_engine *eng, const uint64_t *cts, uint32_t count, uint64_t *glwes_host);
/* Device buffers (what fhe_ks_pbs_batch_dev / fhe_plan_run_batch_dev write); asynchronous on the engine's stream.
 * With a throughput mode on (fhe_engine_set_pipeline 1 or 2) the producing calls run on other streams: the call then
 * waits on the host for all of them first and ends the pipelined run, like a serial call does; the packing itself is
 * still only enqueued. */
int fhe_engine_pack_lwes_dev(fhe_engine *eng, const uint64_t *d_cts, uint32_t count, uint64_t *d_glwes);
/* What the last packing launch ran, recorded on the host when it was enqueued: info[0] 1 once a launch ran, info[1]
 * 32-row tiles per workgroup (1, 2, 4 or 8), info[2] K chunks (grid.z; FHESTR_KS_CHUNKS overrides as for the
 * keyswitch), info[3] K steps per chunk, info[4] K steps in all. */
int fhe_engine_packing_info(fhe_engine *eng, uint32_t info[5]);

/* ---- ring packing: the same packed GLWEs through log2(N) automorphism keys ---------------------------
 * The repacking of Chen, Dai, Kim and Song ("Efficient homomorphic conversion between (ring) LWE ciphertexts", 2021), a
 * second route beside the packing keyswitch for the parameter sets whose matrix key is heavy or refused: the key is
 * log2(N) * k * level GLWE ciphertexts, 39 MB on PARAM_MESSAGE_4_CARRY_4 with five levels.  The output is an ordinary
 * GLWE under the client's GLWE key in the layout above (block j at coefficient j % N of GLWE j / N), so
 * fhe_client_decrypt_packed, sample extraction, the narrow form and the wire forms take it unchanged; the unused
 * coefficients of a short group hold noise around 0, not exact zeros.  All arithmetic mod 2^64:
 *   leaf    every word w of the LWE becomes (w + N/2) >> log2 N (the division that stands in for N^-1 mod 2^64);
 *           A_q[0] = a'[qN], A_q[i] = -a'[qN + N - i], B[0] = b', the other body coefficients 0
 *   autoKS  level l = 1 .. log2 N, t = 2^l + 1, sigma_t(P)(X) = P(X^t) in Z[X] / (X^N + 1):
 *           (0, .., 0, sigma_t(B)) - sum_q sum_it digit_it(sigma_t(A_q)) (*) AK[l][q][it], the keyswitch's signed digits
 *           (level L first), (*) the negacyclic product
 *   merge   pack(0, {ct}) = ct; e = pack(l - 1, even-indexed), o = pack(l - 1, odd-indexed), s = N / 2^l:
 *           pack(l, cts) = (e + X^s o) + autoKS_l(e - X^s o); an absent leaf is the zero ciphertext, a node without a
 *           leaf costs nothing.  c <= N blocks cost sum_{d < log2 N} min(2^d, c) automorphism keyswitches.
 *   key     [log2 N][k][level, level L first][k+1][N] u64: AK[l][q][it] is a GLWE encryption under S of
 *           S_q(X^t) << (64 - base_log * (L - it)), noise glwe_std
 * The products are exact (balanced base-256 planes of the key, one negacyclic number-theoretic transform mod
 * P = 2^32 - 2^20 + 1, centred lift): a pair is admitted while k * level * N * 2^(base_log - 1) * 128 < P / 2, with
 * 1 <= base_log <= 32, level <= 16, base_log * level <= 63, N a power of two in 4 .. 32768.  Host and GPU give the same
 * words.  Noise: a packed coefficient carries its LWE's own noise plus (N^2 / 3) V_aks, V_aks = k N level (2^(2 base_log)
 * + 2) / 12 glwe_std^2 + (k N / 2) 2^(-2 base_log level) / 12. */
/* Fewest levels, then largest base, under the one-prime bound, for which a packed PBS output decoded at delta / 2 stays
 * within the failure bound of fhe_packing_default_params. */
int fhe_ring_packing_default_params(const fhe_params_t *params, fhe_packing_params_t *out);
size_t fhe_ring_packing_key_len(const fhe_params_t *params, const fhe_packing_params_t *pp);   /* words; 0 = refused */
/* out[0]: variance of a raw block extracted from a ring-packed PBS output in nominal units, out[1]: the PBS-input budget
 * (the shape of fhe_packing_unpack_noise).  fhe_ring_narrow_noise: the shape of fhe_narrow_noise. */
int fhe_ring_packing_noise(const fhe_params_t *params, const fhe_packing_params_t *pp, double out[2]);
int fhe_ring_narrow_noise(const fhe_params_t *params, const fhe_packing_params_t *pp, uint32_t bits, double out[3]);
/* automorphism keyswitches of packing `count` LWEs: the cost formula, summed over the GLWEs */
uint64_t fhe_ring_pack_keyswitches(const fhe_params_t *params, uint32_t count);
/* ChaCha20 under `seed`, one stream per (tree level, key polynomial): the same key whatever `threads` is. */
int fhe_client_gen_ring_packing_key(fhe_client_key *ck, const fhe_packing_params_t *pp, const uint8_t seed[32],
                                    uint64_t *key_out, int threads);
/* The definition on the host, with the transform as its exact product (parity; callers without a GPU). */
int fhe_ring_pack_host(const fhe_params_t *params, const fhe_packing_params_t *pp, const uint64_t *key, const uint64_t *cts,
                       uint32_t count, uint64_t *glwes);
/* The host transform on its own: `count` polynomials of N residues below P, in place; forward takes natural order to
 * bit-reversed order, inverse = 1 takes that back.  fhe_ring_product_host: sum over `terms` of a[t] (*) b[t] for
 * polynomials of N signed coefficients, exact while the true magnitude stays below P / 2. */
int fhe_ring_ntt_host(uint32_t N, int inverse, uint32_t *polys, uint32_t count);
int fhe_ring_product_host(uint32_t N, uint32_t terms, const int32_t *a, const int32_t *b, int64_t *out);
/* Upload the key and rewrite it once into transformed digit planes (csrc/ring_packing_kernels.hip.h; 4 x the key's
 * bytes stay resident, the 64-bit form is released); replaces a ring key loaded before, leaves a matrix key alone. */
int fhe_engine_load_ring_packing_key(fhe_engine *eng, const fhe_packing_params_t *pp, const uint64_t *key);
/* fhe_engine_pack_lwes / _dev through the ring route, under the same contract on streams.  Scratch is bounded: the
 * leaves take count * (k+1) * N words and at most 2 GiB (4,096 LWEs at N = 32768), a longer list is refused -- pack it
 * in parts of whole GLWEs; a tree level's merges run in batches of at most 256 MiB of intermediates. */
int fhe_engine_ring_pack_lwes(fhe_engine *eng, const uint64_t *cts, uint32_t count, uint64_t *glwes_host);
int fhe_engine_ring_pack_lwes_dev(fhe_engine *eng, const uint64_t *d_cts, uint32_t count, uint64_t *d_glwes);
/* What the last ring packing call enqueued: info[0] 1 once a call ran, info[1] tree levels, info[2] automorphism
 * keyswitches, info[3] kernel launches, info[4] scratch bytes held. */
int fhe_engine_ring_pack_info(fhe_engine *eng, uint64_t info[5]);
/* The device transform on its own, host arrays in place; synchronises.  Equals fhe_ring_ntt_host word for word. */
int fhe_engine_ring_ntt(fhe_engine *eng, uint32_t N, int inverse, uint32_t *polys, uint32_t count);
/* With only a ring key loaded, the refresh of fhe_engine_unpack_glwes / fhe_engine_unpack_narrow is judged by
 * fhe_ring_packing_noise / fhe_ring_narrow_noise; with a matrix packing key loaded, by that key's pair as before. */

/* ---- packed GLWE ciphertexts as inputs: sample extraction at any coefficient -----------------------
 * The inverse of the packing above, extract_lwe_sample_from_glwe_ciphertext of the reference
 * (core_crypto/algorithms/glwe_sample_extraction.rs:91-147): block j of packed results is coefficient c = j % N of GLWE
 * j / N, and under the flattened GLWE key -- the big LWE key every operation reads -- it is the LWE with
 *     mask[q N + i] = A_q[c - i] for i <= c,  -A_q[N + c - i] for i > c        (q < k),        body = B[c].
 * No key is involved and nothing is rounded: host and GPU give the same words.
 *   input  GLWEs of [k+1][N] u64 (what fhe_engine_pack_lwes writes, or fhe_wire_read_glwe_list returns)
 *   output rows first .. first + count - 1 as count x (kN+1) words
 * The GLWEs must hold block first + count - 1: ceil((first + count) / N) of them is the caller's contract, it cannot be
 * checked here.  count == 0 succeeds and touches nothing. */
/* The plain loop on the host (parity; callers without a GPU). */
int fhe_glwe_sample_extract_host(const fhe_params_t *params, const uint64_t *glwes, uint32_t first, uint32_t count, uint64_t *cts);
/* Noise of a block extracted from a packed PBS output, by the model fhe_packing_default_params judges with: out[0] its
 * variance in nominal units (1 + packing keyswitch variance / V_pbs of fhe_noise_model), out[1] the default PBS-input
 * budget (fhe_noise_model's out[4]).  A plan's inputs are declared nominal, so extracted blocks are refreshed first. */
int fhe_packing_unpack_noise(const fhe_params_t *params, const fhe_packing_params_t *pp, double out[2]);
/* On the GPU (csrc/glwe_extract_kernels.hip.h).  refresh = 0: the raw extracted LWEs.  refresh = 1: every extracted block
 * then goes through one keyswitch + PBS with the identity table over the whole message-and-carry space (the batch path
 * of fhe_ks_pbs_batch_dev, server keys required): the blocks carry nominal noise again and are valid inputs of every plan.
 * The refresh is judged with the decomposition of the loaded packing key: refused when no packing key is loaded, and
 * when out[0] > out[1] of fhe_packing_unpack_noise; the reason is in fhe_last_error.  refresh = 0 needs no key at all.
 * fhe_engine_unpack_glwes: host GLWEs in, host ciphertexts out; synchronises.
 * _dev: device buffers, asynchronous on the engine's stream under the contract of fhe_engine_pack_lwes_dev (a throughput
 * mode makes the call wait for every stream first); the first refresh on an engine uploads the identity table and
 * waits for that copy.  d_cts is what fhe_ks_pbs_batch_dev and fhe_plan_run_batch_dev read; it needs 8-byte alignment
 * only. */
int fhe_engine_unpack_glwes(fhe_engine *eng, const uint64_t *glwes_host, uint32_t first, uint32_t count, int refresh,
                            uint64_t *cts_host);
int fhe_engine_unpack_glwes_dev(fhe_engine *eng, const uint64_t *d_glwes, uint32_t first, uint32_t count, int refresh,
                                uint64_t *d_cts);
/* What the last extraction launched, recorded on the host when it was enqueued: info[0] 1 once a launch ran, info[1]
 * rows (= count), info[2] workgroups, info[3] 1 if the rows were refreshed. */
int fhe_engine_unpack_info(fhe_engine *eng, uint32_t info[4]);

/* ---- narrow packed results: b-bit coefficients, only the coefficients that hold a block -------------
 * The project's own form (the reference has no counterpart; csrc/glwe_narrow.h).  A packed GLWE's modulus is switched
 * down to 2^b, the body coefficients that hold no block are dropped and the rest is bit-packed.  For a width
 * 8 <= b <= 32:
 *     narrow_b(x) = ((x + 2^(63-b)) >> (64-b)) mod 2^b     round to nearest, ties upwards; words within 2^(63-b) of 2^64
 *                                                          wrap to 0
 *     widen_b(v)  = v << (64-b)
 * A packed list of `held` blocks has G = ceil(held / N) GLWEs of [k+1][N] u64 (what fhe_engine_pack_lwes writes); GLWE g
 * holds m_g = min(N, held - g N) blocks.  Its narrow form is a bit stream of kN + m_g fields of b bits each:
 *   field f     narrow_b of word f of the GLWE -- the body follows the mask, so the fields are its first kN + m_g words
 *   bit t       of the stream is bit (t & 63) of u64 word t >> 6; the unused high bits of a stream's last word are 0
 *   stream g    starts at word g W of the list, W = ceil((kN + N) b / 64); the last one has ceil((kN + m_g) b / 64) words
 * so any field is addressed from (g, f, b) alone and two equal lists are equal byte for byte.  A 256-character string
 * under PARAM_MESSAGE_2_CARRY_2 (1,024 blocks) takes (2048 + 1024) * 16 / 8 = 6,144 bytes at 16 bits and 4,992 at 13,
 * against 32,768 packed.  Widening gives full GLWEs whose body coefficients past m_g are 0: they encrypt nothing and
 * nobody reads them.  Everything here is exact integer arithmetic: host and GPU give the same words.
 * Noise: narrowing adds V_narrow(b) = (1 + kN/2) / 12 * 2^(-2b) (torus units) to an extracted block's phase, the
 * average-case form of the modulus switch's term. */
/* out[0]: fhe_packing_unpack_noise's out[0] + V_narrow(bits) / V_pbs, the nominal variance of a block extracted from a
 * narrowed packed PBS output; out[1]: the PBS-input budget; out[2]: log2 of the probability that the client decodes such
 * a coefficient wrongly at delta / 2 (the model fhe_packing_default_params judges with, V_narrow added to the packing's
 * term). */
int fhe_narrow_noise(const fhe_params_t *params, const fhe_packing_params_t *pp, uint32_t bits, double out[3]);
/* The smallest width in 8 .. 32: operand = 1, with out[0] <= out[1] (the narrow list may come back as an operand:
 * fhe_engine_unpack_narrow with refresh); operand = 0, whose out[2] meets the failure bound of
 * fhe_packing_default_params (a result for the client).  Refused, naming the pair, when no width qualifies. */
int fhe_narrow_default_bits(const fhe_params_t *params, const fhe_packing_params_t *pp, int operand, uint32_t *bits);
size_t fhe_narrow_len(const fhe_params_t *params, uint32_t held, uint32_t bits);   /* u64 words of the list; 0 = refused */
/* The plain loops on the host (parity; callers without a GPU).  glwes: ceil(held / N) full GLWEs; narrow: fhe_narrow_len
 * words.  fhe_narrow_sample_extract_host gives rows first .. first + count - 1 as count x (kN+1) words, word for word
 * what fhe_glwe_sample_extract_host gives on fhe_glwe_widen_host's output; first + count > held is refused. */
int fhe_glwe_narrow_host(const fhe_params_t *params, const uint64_t *glwes, uint32_t held, uint32_t bits, uint64_t *narrow);
int fhe_glwe_widen_host(const fhe_params_t *params, const uint64_t *narrow, uint32_t held, uint32_t bits, uint64_t *glwes);
int fhe_narrow_sample_extract_host(const fhe_params_t *params, const uint64_t *narrow, uint32_t held, uint32_t bits,
                                   uint32_t first, uint32_t count, uint64_t *cts);
/* Coefficient j % N of the phase of widened GLWE j / N for j < held, decoded like fhe_client_decrypt_packed. */
int fhe_client_decrypt_narrow(fhe_client_key *ck, const uint64_t *narrow, uint32_t held, uint32_t bits, uint64_t *msgs);
/* On the GPU (csrc/glwe_narrow_kernels.hip.h).  fhe_engine_narrow_glwes: host GLWEs in, host list out; synchronises.
 * _dev: the GLWEs where fhe_engine_pack_lwes_dev wrote them, the list into d_narrow (fhe_narrow_len words, 8-byte
 * aligned); asynchronous on the engine's stream under that call's contract. */
int fhe_engine_narrow_glwes(fhe_engine *eng, const uint64_t *glwes_host, uint32_t held, uint32_t bits, uint64_t *narrow_host);
int fhe_engine_narrow_glwes_dev(fhe_engine *eng, const uint64_t *d_glwes, uint32_t held, uint32_t bits, uint64_t *d_narrow);
/* The way back on the device: the list at d_narrow -> ceil(held / N) full GLWEs at d_glwes (what
 * fhe_engine_unpack_glwes_dev reads), bit-identical to fhe_glwe_widen_host; same contract. */
int fhe_engine_widen_narrow_dev(fhe_engine *eng, const uint64_t *d_narrow, uint32_t held, uint32_t bits, uint64_t *d_glwes);
/* Sample extraction straight from the narrow list: the rows fhe_engine_unpack_glwes gives on the widened GLWEs, under
 * its contract on streams, throughput modes and alignment.  first + count > held is refused (here it can be checked).
 * refresh = 1 is judged with fhe_narrow_noise for the loaded packing key's pair and `bits`: refused when no packing key
 * is loaded or when out[0] > out[1]; the reason is in fhe_last_error.  The host form uploads only the streams the range
 * touches.  These calls leave fhe_engine_unpack_info as it was. */
int fhe_engine_unpack_narrow(fhe_engine *eng, const uint64_t *narrow_host, uint32_t held, uint32_t bits, uint32_t first,
                             uint32_t count, int refresh, uint64_t *cts_host);
int fhe_engine_unpack_narrow_dev(fhe_engine *eng, const uint64_t *d_narrow, uint32_t held, uint32_t bits, uint32_t first,
                                 uint32_t count, int refresh, uint64_t *d_cts);
/* What the last of the five calls above launched, recorded on the host when it was enqueued: info[0] 1 once a launch
 * ran, info[1] the kernel (1 = narrowing, 2 = extraction, 3 = widening), info[2] list words written / rows extracted /
 * GLWE words written, info[3] workgroups, info[4] bits. */
int fhe_engine_narrow_info(fhe_engine *eng, uint32_t info[5]);

/* ---- transciphering: strings encrypted under a stream cipher, the keystream removed on the GPU ----------
 * The client encrypts its string with Trivium or Kreyvium (1 byte per character plus the IV) and uploads the cipher's
 * key BITS as big-key LWE ciphertexts once (80 or 128 of them, each a 0 or a 1; any input path carries them).  The
 * server generates the keystream homomorphically, 64 steps per lookup level, and removes it: what comes out are the block
 * ciphertexts every fhe_str_* call takes (the reference's apps/trivium, trivium_shortint.rs / kreyvium_shortint.rs, on
 * this engine's batched PBS).  Definition, tables and noise: csrc/stream_cipher.h, csrc/transcipher.h.
 *
 * Trivium is an 80-bit cipher: it is offered for its published test vectors and for parity with the reference.
 * Kreyvium is the one whose 128-bit key matches the 128-bit parameter sets.
 *
 * Bit order (the reference's and the published vectors'): a key or IV of L = 80 / 128 bits is given as L / 8 bytes, the bit
 * array is x[8 j + l] = bit l (LSB first) of byte j, spec bit K_j (1 .. L) is x[L - j]; keystream bit 8 j + l is bit l
 * of keystream byte j. */
#define FHE_STREAM_TRIVIUM 1u
#define FHE_STREAM_KREYVIUM 2u
/* info[0] key bits, info[1] IV bits, info[2] warm-up steps discarded before the first keystream bit (1152) */
int fhe_stream_cipher_info(uint32_t cipher, uint32_t info[3]);
/* Keystream bytes first_byte .. first_byte + n_bytes - 1 in the clear (client side, host only). */
int fhe_stream_cipher_keystream(uint32_t cipher, const uint8_t *key, const uint8_t *iv, uint64_t first_byte, uint8_t *out,
                                size_t n_bytes);
/* 0 if the parameter set can run the cipher homomorphically, else 1 with the reason in fhe_last_error.  Needs no device.
 * Supported: msg_mod * carry_mod >= 16 (a state update feeds a lookup values up to 14), log2(msg_mod) divides 8, and the
 * noise model puts every lookup input (35 or 54 nominal variances for a state update, 6 or 7 for the keystream) within
 * the plans' default PBS-input budget. */
int fhe_transcipher_supported(const fhe_params_t *params, uint32_t cipher);
/* Table number `table` (0 .. *n_tables - 1: f_3, 1 - f_3, f_4, 1 - f_4, then g_{i,c} at 4 + 2 i + c) over the
 * msg_mod * carry_mod message-and-carry values.  values may be NULL to read *n_tables only. */
int fhe_transcipher_table(const fhe_params_t *params, uint32_t table, uint64_t *values, uint32_t *n_tables);
/* The round on the host, plain loops (csrc/transcipher.cpp): the pin of the kernels, and what a test runs on trivial
 * ciphertexts.  ring: fhe_transcipher_ring_len words (4 slots x streams x 256 rows); key: L rows K_1 .. K_L; ivs:
 * streams x L / 8 bytes.  init writes the blocks of rounds -1 and -2.  gather writes the streams x rows (192 warm-up, 256
 * data) lookup inputs of round `round` (>= 0; data rounds start at 18) and their table numbers; the lookups' outputs
 * belong in ring slot round mod 4, streams x rows rows back to back from word (round mod 4) x streams x 256 x (kN + 1).
 * data: streams x n_bytes clear cipher bytes of one fhe_transcipher_next call, m the round within that call.  apply sums
 * the keystream lookups of data round `round` into the blocks of characters 8 m .. of out (streams x n_bytes x
 * blocks-per-character rows). */
size_t fhe_transcipher_ring_len(const fhe_params_t *params, uint32_t streams);
int fhe_transcipher_init_host(const fhe_params_t *params, uint32_t cipher, uint32_t streams, const uint64_t *key,
                              const uint8_t *ivs, uint64_t *ring);
int fhe_transcipher_gather_host(const fhe_params_t *params, uint32_t cipher, uint32_t streams, int32_t round, uint32_t rows,
                                const uint64_t *ring, const uint64_t *key, const uint8_t *ivs, const uint8_t *data,
                                uint32_t n_bytes, uint32_t m, uint64_t *pbs_in, uint32_t *tables);
int fhe_transcipher_apply_host(const fhe_params_t *params, uint32_t cipher, uint32_t streams, int32_t round,
                               const uint64_t *ring, uint32_t n_bytes, uint32_t m, uint64_t *out);
/* The same three through the kernels (csrc/transcipher_kernels.hip.h), host arrays in and out, one launch each;
 * synchronise.  Word for word what the host loops give. */
int fhe_engine_transcipher_init(fhe_engine *eng, uint32_t cipher, uint32_t streams, const uint64_t *key, const uint8_t *ivs,
                                uint64_t *ring);
int fhe_engine_transcipher_gather(fhe_engine *eng, uint32_t cipher, uint32_t streams, int32_t round, uint32_t rows,
                                  const uint64_t *ring, const uint64_t *key, const uint8_t *ivs, const uint8_t *data,
                                  uint32_t n_bytes, uint32_t m, uint64_t *pbs_in, uint32_t *tables);
int fhe_engine_transcipher_apply(fhe_engine *eng, uint32_t cipher, uint32_t streams, int32_t round, const uint64_t *ring,
                                 uint32_t n_bytes, uint32_t m, uint64_t *out);

/* One cipher key on one engine (server keys loaded), for up to max_streams strings at a time.  key_cts: host rows, the
 * encryptions of the key bits in spec order K_1 .. K_L; they are made resident.  Owned by the engine: its device memory goes with the
 * engine at the latest; call fhe_transcipher_destroy before fhe_engine_destroy, the handle must not be used after it.  Every call below takes the engine's lock and ends a pipelined run like any serial path. */
typedef struct fhe_transcipher fhe_transcipher;
int fhe_transcipher_create(fhe_engine *eng, uint32_t cipher, const uint64_t *key_cts, uint32_t max_streams,
                           fhe_transcipher **out);
int fhe_transcipher_destroy(fhe_transcipher *tc);
/* Start n_streams <= max_streams strings, stream s under IV ivs[s L / 8 ..]: the initial state and the 18 warm-up rounds,
 * all streams in lockstep, one lookup level of n_streams x 192 inputs per round.  Asynchronous on the engine's stream.
 * May be called again: it starts over. */
int fhe_transcipher_begin(fhe_transcipher *tc, const uint8_t *ivs, uint32_t n_streams);
/* The next n_bytes characters of every stream.  data: n_streams x n_bytes clear cipher bytes, string s at data[s n_bytes ..].
 * Result: n_streams x n_bytes x blocks-per-character big-key block ciphertexts in the layout of an encrypted string,
 * to exactly one of out_host (synchronises) and d_out (asynchronous on the engine's stream).
 * EVERY CALL STARTS ON AN 8-BYTE KEYSTREAM BOUNDARY and consumes ceil(n_bytes / 8) rounds of 64 keystream bits: the
 * keystream bytes a call leaves over are skipped.  The client passes the matching offset -- 8 x the rounds consumed so
 * far, info[7] of fhe_transcipher_info -- when it encrypts the bytes of the next call.
 * refresh = 1 (the default of the Python layer): the blocks, sums of log2(msg_mod) lookups each, go through one more
 * lookup level with the identity table and come out as nominal plan inputs.  refresh = 0 leaves them at log2(msg_mod)
 * nominal variances. */
int fhe_transcipher_next(fhe_transcipher *tc, const uint8_t *data, uint32_t n_bytes, int refresh, uint64_t *out_host,
                         uint64_t *d_out);
/* info[0] cipher, [1] max_streams, [2] streams of the current run (0 before begin), [3] warm-up rounds and [4] data rounds
 * since begin, [5] / [6] low / high word of the lookups since begin (all streams, refreshes included), [7] the keystream
 * byte the next call starts at. */
int fhe_transcipher_info(fhe_transcipher *tc, uint32_t info[8]);
/* Per-phase device times of the data rounds, for measurement (scripts/transcipher_timing.py): on = 1 makes every data
 * round end in a synchronisation and accumulates ms[0] gather, ms[1] keyswitch + PBS, ms[2] apply over *rounds rounds
 * since begin.  ms / rounds may be NULL to switch only. */
int fhe_transcipher_timing(fhe_transcipher *tc, int on, double ms[3], uint32_t *rounds);

/* ---- casting keys: blocks move between clients and between parameter sets ---------------------------
 * shortint::KeySwitchingKey of the reference (shortint/key_switching_key/mod.rs, parameters/key_switching.rs): an LWE
 * keyswitch key from the SOURCE client's big LWE key (k N words of cp.src) to a key of the DESTINATION client, whose
 * engine then serves the source's blocks.  Definition, noise and the host loop: csrc/cast.h, csrc/cast.cpp; the device
 * side: csrc/cast_dev.hip, csrc/cast_kernels.hip.h.
 *   FHE_CAST_TO_BIG    the reference's form: to the destination's big key, noise of the destination's lwe_std
 *                      (new_key_switching_key); default decomposition (1, 15), the constant of
 *                      PARAM_KEYSWITCH_1_1_KS_PBS_TO_2_2_KS_PBS.  A cast is this keyswitch and, where a table follows
 *                      (below), one ordinary keyswitch + PBS level.
 *   FHE_CAST_TO_SMALL  the project's own form: straight to the destination's small key, so that the cast block feeds
 *                      the blind rotation directly: one lookup level in all.  Defaults to the destination's own
 *                      (ks_base_log, ks_level).
 *   key    [src k N][level, level L first][out_dim + 1] u64, out_dim = the destination's k N or n: the layout of
 *          LweKeyswitchKey, which fhe_wire_write_keyswitch_key / fhe_wire_read_keyswitch_key carry
 * Refused, with the reason in fhe_last_error: more than 16 levels, base_log above 7, base_log * level above 63, a key
 * above 4 GiB, message-and-carry moduli that are not powers of two.  fhe_cast_key_len returns 0 then. */
#define FHE_CAST_TO_BIG 0u
#define FHE_CAST_TO_SMALL 1u
typedef struct fhe_cast_params_t {
    fhe_params_t src;          /* the source client's parameter set */
    uint32_t base_log, level;  /* decomposition of the cast key */
    uint32_t target;           /* FHE_CAST_TO_BIG / FHE_CAST_TO_SMALL */
} fhe_cast_params_t;
int fhe_cast_default_params(const fhe_params_t *src, const fhe_params_t *dst, uint32_t target, fhe_cast_params_t *cp);
size_t fhe_cast_key_len(const fhe_params_t *dst, const fhe_cast_params_t *cp);   /* words; 0 = refused */
/* cast_rshift of the reference (mod.rs:62-80): log2 of the destination's msg_mod * carry_mod minus log2 of the source's. */
int fhe_cast_rshift(const fhe_params_t *src, const fhe_params_t *dst, int32_t *shift);
/* The key, by the routine that generates the clients' own keyswitch keys: row (i, l) encrypts source key bit i shifted to
 * level l under the destination's key of cp->target.  ck_src must have been created with cp->src.  out: fhe_cast_key_len
 * words.  `seed` drives masks and noise. */
int fhe_client_gen_cast_key(fhe_client_key *ck_src, fhe_client_key *ck_dst, const fhe_cast_params_t *cp,
                            const uint8_t seed[32], uint64_t *out);
/* The keyswitch in plain loops (the pin of the kernels): count rows of src k N + 1 words -> count rows of out_dim + 1. */
int fhe_cast_host(const fhe_params_t *dst, const fhe_cast_params_t *cp, const uint64_t *key, const uint64_t *in,
                  uint32_t count, uint64_t *out);
/* Noise of a keyswitched block, by the keyswitch terms of fhe_noise_model at the cast key's dimensions.  v_in: the
 * source block's variance in units of the SOURCE set's nominal (PBS output) variance.  out[0]: what the destination's
 * next lookup sees, in units of the destination's nominal variance -- TO_BIG: the block itself; TO_SMALL: the input of
 * equal effect, (torus variance - the destination's own keyswitch term) / V_pbs.  out[1]: the destination's default
 * PBS-input budget.  out[2]: the keyswitched block's variance with the torus as unit. */
int fhe_cast_noise(const fhe_params_t *dst, const fhe_cast_params_t *cp, double v_in, double out[3]);

/* One cast key on the destination's engine; an engine may hold many (one per source client).  The words go up once and
 * are rewritten into the matrix-core keyswitch's digit planes (csrc/ks_mfma_kernels.hip.h).  Owned by the engine like a
 * fhe_transcipher: destroy it before the engine, never use it after. */
typedef struct fhe_cast_key fhe_cast_key;
int fhe_cast_key_create(fhe_engine *eng, const fhe_cast_params_t *cp, const uint64_t *key, fhe_cast_key **out);
int fhe_cast_key_destroy(fhe_cast_key *h);
/* info[0] target, [1] base_log, [2] level, [3] source k N, [4] out_dim, [5] shift + 64, [6] 1 if packed inputs take the
 * fused digit kernel, [7] what the last cast launched: 0 nothing, 1 digits from LWEs, 2 fused digits from GLWEs,
 * 3 extraction + digits. */
int fhe_cast_key_info(fhe_cast_key *h, uint32_t info[8]);
/* Packed inputs: 1 (default) cast_decompose_glwe_kernel writes the digits straight from the GLWEs; 0 the GLWEs are
 * extracted to LWEs first (fhe_engine_unpack_glwes_dev's kernel).  Same results; for measurement and tests. */
int fhe_cast_key_set_fused(fhe_cast_key *h, int on);
/* Regrouping for strings cast to a set with more message bits per block: `group` consecutive source blocks, least
 * significant first, become ONE destination block.  The keyswitched rows are combined as sum_i msg_src^i * row_i before
 * the single table x -> x >> shift, so a destination block costs one lookup; count must then be a multiple of group
 * and count / group blocks come out.  Refused unless msg_src^group is the destination's msg_mod and the largest lookup
 * input, (msg_src^group - 1) << shift, stays inside the destination's message-and-carry space: 1_1 -> 2_2 and
 * 2_2 -> 4_4 (group 2) qualify, 1_1 -> 4_4 (group 4: up to 960 against 255) does not.  group = 1 switches it off. */
int fhe_cast_key_set_group(fhe_cast_key *h, uint32_t group);
/* The rule above without an engine: *degree the largest lookup input, *space the destination's msg_mod * carry_mod;
 * returns 1 with the reason when the regrouping is refused. */
int fhe_cast_regroup_check(const fhe_params_t *src, const fhe_params_t *dst, uint32_t group, uint64_t *degree, uint64_t *space);
/* What the source blocks are declared to carry, in the source set's nominal units, for the refusal below: 1 (default) for
 * the outputs of a lookup, 0 for fresh encryptions; a block of a packed lookup output carries out[0] of
 * fhe_packing_unpack_noise for the SOURCE's set and packing pair, of a narrow list out[0] of fhe_narrow_noise.  Like a
 * plan's inputs it is a declaration. */
int fhe_cast_key_set_input_noise(fhe_cast_key *h, double v_in);
/* count source blocks -> count destination big-key blocks.  After the keyswitch:
 *   TO_BIG,   shift > 0   one keyswitch + PBS with the table x -> x >> shift                  (mod.rs:107-127)
 *   TO_BIG,   shift == 0  FHE_CAST_RAW: nothing more, the reference's behaviour; FHE_CAST_REFRESH: the identity table
 *   TO_SMALL              always the blind rotation with that table
 *   FHE_CAST_KEYSWITCHED  the keyswitched rows alone, out_dim + 1 words each (what fhe_cast_host gives)
 * A cast that ends in a table is refused when fhe_cast_noise at the declared input noise puts out[0] above out[1] (the
 * reference's own (1, 15) key from 1_1 to 2_2 is: 1,126 nominal variances against a budget of 138; its two steps stay
 * available unguarded as FHE_CAST_KEYSWITCHED followed by fhe_ks_pbs_batch).  shift < 0, a cast to
 * fewer bits, needs the SOURCE server key first (mod.rs:128-140): one lookup with x -> (x << -shift) % (msg * carry) on
 * the source's engine, Engine.cast_prepare of the Python layer; blocks that skipped it cannot be told apart here.
 * fhe_cast_lwes: host rows in and out, synchronises.  _dev: device buffers, asynchronous on the engine's stream under the
 * contract of fhe_engine_unpack_glwes_dev. */
#define FHE_CAST_RAW 0
#define FHE_CAST_REFRESH 1
#define FHE_CAST_KEYSWITCHED 2
int fhe_cast_lwes(fhe_cast_key *h, const uint64_t *in, uint32_t count, int mode, uint64_t *out);
int fhe_cast_lwes_dev(fhe_cast_key *h, const uint64_t *d_in, uint32_t count, int mode, uint64_t *d_out);
/* The same for blocks first .. first + count - 1 of the source's packed GLWEs ([src k + 1][src N], block j = coefficient
 * j % N of GLWE j / N).  The GLWE key flattened is the big LWE key, so nothing is unpacked under the old key: the digits
 * of the sample-extracted rows are written straight from the GLWEs.  The host form takes the GLWEs from GLWE 0 on. */
int fhe_cast_packed(fhe_cast_key *h, const uint64_t *glwes, uint32_t first, uint32_t count, int mode, uint64_t *out);
int fhe_cast_packed_dev(fhe_cast_key *h, const uint64_t *d_glwes, uint32_t first, uint32_t count, int mode, uint64_t *d_out);
/* The same for the source's narrow list of `held` blocks at `bits` bits (fhe_engine_narrow_glwes on the source's side):
 * the list is widened on the device at the source's (k, N) -- the kernel of fhe_engine_widen_narrow_dev -- and cast as
 * packed GLWEs; nothing of it is widened on the host.  The list starts at its first stream; first + count > held is refused. */
int fhe_cast_narrow(fhe_cast_key *h, const uint64_t *narrow, uint32_t held, uint32_t bits, uint32_t first, uint32_t count,
                    int mode, uint64_t *out);
int fhe_cast_narrow_dev(fhe_cast_key *h, const uint64_t *d_narrow, uint32_t held, uint32_t bits, uint32_t first,
                        uint32_t count, int mode, uint64_t *d_out);
/* The digit fragments of a batch as the product reads them ([row tile][step][lane][16] int8, ceil(count / 32) * steps KB;
 * *bytes receives that size, out may be NULL to query it): from LWE rows (packed = 0) or from packed GLWEs through the
 * kernel fhe_cast_key_set_fused selects.  Host arrays; synchronises.  What tests compare byte for byte. */
int fhe_cast_debug_digits(fhe_cast_key *h, const uint64_t *src, uint32_t first, uint32_t count, int packed, int8_t *out,
                          size_t *bytes);

/* ---- tfhe-rs wire format (serde + bincode 1.x, fixed-width little endian) ---------------------- */
/* Byte forms of core_crypto's LweCiphertext<Vec<u64>>, LweKeyswitchKey<Vec<u64>>, standard-domain
 * LweBootstrapKey<Vec<u64>> and shortint::Ciphertext as tfhe-rs 0.5 writes them with bincode::serialize /
 * safe_serialize (entities/lwe_ciphertext.rs:500-507, lwe_keyswitch_key.rs:76-86,
 * lwe_bootstrap_key.rs:98-106 + ggsw_ciphertext_list.rs:9-20, commons/ciphertext_modulus.rs:41-64,
 * shortint/ciphertext/mod.rs:261-270, safe_deserialization.rs:16-99).  Native modulus 2^64 only.
 * Writers: `out` may be NULL to query the size; *written receives the byte count either way.
 * Readers validate every dimension against the parameter set (the reference's ParameterSetConformant)
 * and never read past in_len.  The reference ships no serialized fixture: parity unpinned. */
typedef struct fhe_shortint_meta {
    uint64_t degree, noise_level, message_modulus, carry_modulus;
    uint32_t pbs_order;   /* 0 = KeyswitchBootstrap, 1 = BootstrapKeyswitch (commons/parameters.rs:233-245) */
} fhe_shortint_meta;
int fhe_wire_write_lwe_ciphertext(const uint64_t *ct, size_t lwe_size, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_lwe_ciphertext(const uint8_t *in, size_t in_len, uint64_t *ct, size_t ct_cap, size_t *lwe_size,
                                 size_t *consumed);
int fhe_wire_write_keyswitch_key(const fhe_params_t *p, const uint64_t *ksk, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_keyswitch_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *ksk, size_t *consumed);
int fhe_wire_write_bootstrap_key(const fhe_params_t *p, const uint64_t *bsk_std, uint8_t *out, size_t out_cap,
                                 size_t *written);
int fhe_wire_read_bootstrap_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *bsk_std,
                                size_t *consumed);
/* safe_framing != 0: the version / type-name header of safe_serialize; size_limit (0 = none) bounds the
 * object's bytes like safe_deserialize's serialized_size_limit */
int fhe_wire_write_shortint_ciphertext(const uint64_t *ct, size_t lwe_size, const fhe_shortint_meta *meta,
                                       int safe_framing, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_shortint_ciphertext(const uint8_t *in, size_t in_len, int safe_framing, uint64_t size_limit,
                                      uint64_t *ct, size_t ct_cap, size_t *lwe_size, fhe_shortint_meta *meta,
                                      size_t *consumed);

/* ---- seeded ("compressed") server keys -------------------------------------------------------
 * What a tfhe-rs client sends: shortint CompressedServerKey = SeededLweKeyswitchKey + SeededLweBootstrapKey
 * (or SeededLweMultiBitBootstrapKey), shortint/server_key/compressed.rs.  A seeded key holds the bodies only
 * (keyswitch key: k*N*ks_level words; bootstrap key: n_ggsw*pbs_level*(k+1) polynomials of N words) and a
 * 128-bit compression seed; the masks are the seed's AES-128-CTR stream (concrete-csprng) in storage order
 * (seeded_lwe_keyswitch_key_decompression.rs, seeded_lwe_bootstrap_key_decompression.rs,
 * seeded_lwe_multi_bit_bootstrap_key_decompression.rs; details in csrc/seeded_keys.cpp).
 * fhe_seeded_decompress_* rebuild the standard-domain keys fhe_engine_load_keys takes; fhe_seeded_split_* are
 * the inverse (bodies of a standard key); fhe_seeded_mask_words exposes the mask stream (tests, and clients that
 * want to ENCRYPT seeded keys).  The AES block function carries the FIPS-197 vector the reference tests with;
 * stream position, integer packing and draw order follow the reference's sources: parity with a real client
 * is unpinned (no seeded fixture in the reference). */
/* The device-side route: upload the bodies only and expand both mask streams on the GPU (csrc/seeded_kernels.hip.h),
 * then install like fhe_engine_load_keys.  bsk_std_out / ksk_out (may be NULL) receive the standard-domain keys --
 * bit-identical to fhe_seeded_decompress_*. */
int fhe_engine_load_seeded_keys(fhe_engine *eng, const uint8_t ksk_seed[16], const uint64_t *ksk_bodies,
                                const uint8_t bsk_seed[16], const uint64_t *bsk_bodies, uint64_t *bsk_std_out,
                                uint64_t *ksk_out);
/* Compressed ciphertexts (shortint CompressedCiphertext: a body and a compression seed EACH, 92 bytes on the wire
 * instead of 8 (kN+1); shortint/ciphertext/mod.rs:471-478, seeded_lwe_ciphertext_decompression.rs): expanded on the
 * GPU into d_out (device, count x (kN+1) words; may be NULL) and / or host_out.  fhe_seeded_decompress_lwe_batch is
 * the host-side twin (any LWE dimension). */
int fhe_engine_expand_seeded_lwe(fhe_engine *eng, const uint8_t *seeds /* [count][16] */, const uint64_t *bodies,
                                 uint32_t count, uint64_t *d_out, uint64_t *host_out);
int fhe_seeded_decompress_lwe_batch(uint32_t lwe_dim, const uint8_t *seeds, const uint64_t *bodies, uint32_t count,
                                    uint64_t *out);
int fhe_wire_write_compressed_ciphertext(uint64_t body, size_t lwe_size, const uint8_t seed[16], const fhe_shortint_meta *meta,
                                         uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_compressed_ciphertext(const uint8_t *in, size_t in_len, uint64_t *body, size_t *lwe_size, uint8_t seed[16],
                                        fhe_shortint_meta *meta, size_t *consumed);
/* integer RadixCiphertext / CompressedRadixCiphertext: Vec of blocks, least significant first
 * (integer/ciphertext/mod.rs:18-21,30,45) -- an FheUint8 character is four blocks under PARAM_MESSAGE_2_CARRY_2. */
int fhe_wire_write_radix_ciphertext(const uint64_t *cts, size_t lwe_size, const fhe_shortint_meta *metas, size_t n_blocks,
                                    uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_radix_ciphertext(const uint8_t *in, size_t in_len, uint64_t *cts, size_t lwe_size, size_t max_blocks,
                                   fhe_shortint_meta *metas, size_t *n_blocks, size_t *consumed);
int fhe_wire_write_compressed_radix_ciphertext(const uint64_t *bodies, const uint8_t *seeds /* [n][16] */, size_t lwe_size,
                                               const fhe_shortint_meta *metas, size_t n_blocks, uint8_t *out, size_t out_cap,
                                               size_t *written);
int fhe_wire_read_compressed_radix_ciphertext(const uint8_t *in, size_t in_len, uint64_t *bodies, uint8_t *seeds,
                                              size_t *lwe_size, size_t max_blocks, fhe_shortint_meta *metas,
                                              size_t *n_blocks, size_t *consumed);
int fhe_aes128_encrypt_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]);
int fhe_seeded_mask_words(const uint8_t seed[16], uint64_t *out, size_t count);
int fhe_seeded_decompress_keyswitch_key(const fhe_params_t *p, const uint8_t seed[16], const uint64_t *bodies, uint64_t *ksk);
int fhe_seeded_decompress_bootstrap_key(const fhe_params_t *p, const uint8_t seed[16], const uint64_t *bodies,
                                        uint64_t *bsk_std);
int fhe_seeded_split_keyswitch_key(const fhe_params_t *p, const uint64_t *ksk, uint64_t *bodies);
int fhe_seeded_split_bootstrap_key(const fhe_params_t *p, const uint64_t *bsk_std, uint64_t *bodies);
/* bincode forms (entities/seeded_lwe_keyswitch_key.rs:11-21, seeded_ggsw_ciphertext_list.rs:12-23,
 * seeded_lwe_multi_bit_bootstrap_key.rs:16-25, lwe_multi_bit_bootstrap_key.rs:11-20); the bootstrap-key
 * functions read / write the multi-bit container when the parameter set has a grouping factor */
int fhe_wire_write_seeded_keyswitch_key(const fhe_params_t *p, const uint8_t seed[16], const uint64_t *bodies, uint8_t *out,
                                        size_t out_cap, size_t *written);
int fhe_wire_read_seeded_keyswitch_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint8_t seed[16],
                                       uint64_t *bodies, size_t *consumed);
int fhe_wire_write_seeded_bootstrap_key(const fhe_params_t *p, const uint8_t seed[16], const uint64_t *bodies, uint8_t *out,
                                        size_t out_cap, size_t *written);
int fhe_wire_read_seeded_bootstrap_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint8_t seed[16],
                                       uint64_t *bodies, size_t *consumed);
/* shortint CompressedServerKey, the object a client serializes for the server (shortint/server_key/compressed.rs:11-17,
 * 44-55): seeded keyswitch key, Classic / MultiBit seeded bootstrap key (by the parameter set's grouping factor),
 * message and carry modulus (checked against the parameter set), max_degree, ciphertext modulus, pbs_order. */
int fhe_wire_write_compressed_server_key(const fhe_params_t *p, const uint8_t ksk_seed[16], const uint64_t *ksk_bodies,
                                         const uint8_t bsk_seed[16], const uint64_t *bsk_bodies, uint64_t max_degree,
                                         uint32_t pbs_order, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_compressed_server_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint8_t ksk_seed[16],
                                        uint64_t *ksk_bodies, uint8_t bsk_seed[16], uint64_t *bsk_bodies,
                                        uint64_t *max_degree, uint32_t *pbs_order, size_t *consumed);
int fhe_wire_write_multi_bit_bootstrap_key(const fhe_params_t *p, const uint64_t *bsk_std, uint8_t *out, size_t out_cap,
                                           size_t *written);
int fhe_wire_read_multi_bit_bootstrap_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *bsk_std,
                                          size_t *consumed);

/* Public-key objects (bincode as above): LweCompactCiphertextList<Vec<u64>> { data, lwe_size, lwe_ciphertext_count,
 * ciphertext_modulus } (entities/lwe_compact_ciphertext_list.rs:18-27); shortint CompactCiphertextList { ct_list,
 * degree, message_modulus, carry_modulus, pbs_order, noise_level } (shortint/ciphertext/mod.rs:521-529); integer
 * CompactCiphertextList { ct_list, num_blocks_per_integer } (integer/ciphertext/mod.rs:71-78); LweCompactPublicKey
 * { glwe_ciphertext: GlweCiphertext { data, polynomial_size, ciphertext_modulus } }, GLWE size 2, polynomial size kN
 * (entities/lwe_compact_public_key.rs:12-17, glwe_ciphertext.rs:286-293).  Readers check lwe_size / polynomial size
 * and the moduli against the parameter set, the container length against the count
 * (lwe_compact_ciphertext_list_size), refuse more than max_count ciphertexts (list: room for
 * fhe_compact_list_len(params, max_count) words) and never read past in_len.  Parity unpinned, as above.  The
 * shortint CompactPublicKey wrapper (it embeds a ShortintParameterSet) is not covered. */
int fhe_wire_write_compact_list(const fhe_params_t *p, const uint64_t *list, uint32_t count, uint8_t *out, size_t out_cap,
                                size_t *written);
int fhe_wire_read_compact_list(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *list, uint32_t max_count,
                               uint32_t *count, size_t *consumed);
/* meta->message_modulus / carry_modulus must be the parameter set's; num_blocks_per_integer == 0 writes / expects the
 * shortint object, > 0 the integer one (count must then be a multiple of it; the reader returns it through
 * *num_blocks_per_integer, which may be NULL for the shortint object only). */
int fhe_wire_write_shortint_compact_list(const fhe_params_t *p, const uint64_t *list, uint32_t count,
                                         const fhe_shortint_meta *meta, uint64_t num_blocks_per_integer, uint8_t *out,
                                         size_t out_cap, size_t *written);
int fhe_wire_read_shortint_compact_list(const fhe_params_t *p, const uint8_t *in, size_t in_len, int integer_form,
                                        uint64_t *list, uint32_t max_count, uint32_t *count, fhe_shortint_meta *meta,
                                        uint64_t *num_blocks_per_integer, size_t *consumed);
int fhe_wire_write_compact_public_key(const fhe_params_t *p, const uint64_t *pk, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_compact_public_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *pk, size_t *consumed);

/* LwePackingKeyswitchKey<Vec<u64>> { data, decomp_base_log, decomp_level_count, output_glwe_size, output_polynomial_size,
 * ciphertext_modulus } (entities/lwe_packing_keyswitch_key.rs) and GlweCiphertext<Vec<u64>> { data, polynomial_size,
 * ciphertext_modulus } (glwe_ciphertext.rs:286-293); a GLWE list is a bincode Vec of them (u64 length first).  Readers
 * check every dimension against the parameter set and the container lengths against them, refuse more than max_glwes
 * ciphertexts and never read past in_len.  Parity unpinned, as above. */
int fhe_wire_write_packing_key(const fhe_params_t *p, const fhe_packing_params_t *pp, const uint64_t *pksk, uint8_t *out,
                               size_t out_cap, size_t *written);
/* pksk may be NULL to read the decomposition only (then size the buffer with fhe_packing_key_len and call again) */
int fhe_wire_read_packing_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, fhe_packing_params_t *pp,
                              uint64_t *pksk, size_t pksk_cap_words, size_t *consumed);
/* The ring packing key in the same layout (data = [log2 N][k][level][k+1][N]); the reader checks the pair against
 * fhe_ring_packing_key_len.  Parity unpinned. */
int fhe_wire_write_ring_packing_key(const fhe_params_t *p, const fhe_packing_params_t *pp, const uint64_t *key, uint8_t *out,
                                    size_t out_cap, size_t *written);
int fhe_wire_read_ring_packing_key(const fhe_params_t *p, const uint8_t *in, size_t in_len, fhe_packing_params_t *pp,
                                   uint64_t *key, size_t key_cap_words, size_t *consumed);
int fhe_wire_write_glwe_ciphertext(const fhe_params_t *p, const uint64_t *glwe, uint8_t *out, size_t out_cap, size_t *written);
int fhe_wire_read_glwe_ciphertext(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *glwe, size_t *consumed);
int fhe_wire_write_glwe_list(const fhe_params_t *p, const uint64_t *glwes, uint32_t n_glwes, uint8_t *out, size_t out_cap,
                             size_t *written);
int fhe_wire_read_glwe_list(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *glwes, uint32_t max_glwes,
                            uint32_t *n_glwes, size_t *consumed);
/* The narrow list ("narrow packed results" above).  This is the project's own container, it has no reference
 * counterpart: glwe_dimension, polynomial_size, bits and held as little-endian u64, then a bincode Vec<u64> of the
 * fhe_narrow_len words.  The reader checks k and N against the parameter set, 8 <= bits <= 32, held <= max_held, the
 * word count against fhe_narrow_len and that every tail bit is 0 (the writer refuses a list with one set), and never
 * reads past in_len.  narrow may be NULL to read *held and *bits only (then size the buffer with fhe_narrow_len and
 * call again); otherwise it has room for narrow_cap_words words. */
int fhe_wire_write_narrow_list(const fhe_params_t *p, const uint64_t *narrow, uint32_t held, uint32_t bits, uint8_t *out,
                               size_t out_cap, size_t *written);
int fhe_wire_read_narrow_list(const fhe_params_t *p, const uint8_t *in, size_t in_len, uint64_t *narrow,
                              size_t narrow_cap_words, uint32_t max_held, uint32_t *held, uint32_t *bits, size_t *consumed);

#ifdef __cplusplus
}
#endif
#endif
