/*
 * msm_hip.h -- C ABI of the MI355X-native BN254 G1 variable-base MSM engine.
 *
 * This is the drop-in boundary for ONE path of zkmopro/gpu-acceleration (mopro-msm v0.2.0):
 *
 *     pub fn metal_variable_base_msm(bases: &[G1Affine], scalars: &[Fr])
 *         -> Result<G1Projective, Box<dyn Error>>          mopro-msm/src/msm/metal_msm/metal_msm.rs:642-695
 *
 * A Rust shim (rust/mopro-msm-hip) keeps that signature and forwards to
 * msm_bn254_g1() below.  Everything the reference does between that call and its return value --
 * MetalMSMPipeline::new / execute_pipeline / final_reduction (metal_msm.rs:48-261), the Metal
 * dispatch layer (host/metal_wrapper.rs:55-217, host/shader_manager.rs:98-167, host/gpu.rs:3-31) and the
 * five kernels (shader/cuzk/{convert_point_coords_and_decompose_scalars,transpose,smvp,pbpr}.metal) -- is
 * replaced by the implementation behind this header.
 *
 * Word formats (pinned by the reference's packer, utils/limbs_conversion.rs:311-378):
 *   field element  = 8 little-endian uint32 words
 *   affine base    = x[8] || y[8]                         (16 words, 64 bytes)
 *   scalar         = 8 words, standard (non-Montgomery) form, value < r
 *   Jacobian point = X[8] || Y[8] || Z[8], Montgomery form (R = 2^256); identity <=> Z == 0
 * MSM_FORM_MONT coordinates are bit-identical to arkworks' internal `Fq.0.0` limbs, so the shim
 * can hand them over without the 3N CPU-side Montgomery reductions of pack_affine_and_scalars.
 *
 * Determinism.  out_affine_std (and out_is_inf) are CANONICAL: the same inputs give the same bits on every call, every entry point, every
 * plan and any number of GPUs -- this is what "bit-exact against arkworks" means here and what every parity test compares.
 * out_jacobian_mont -- the reference's result type, G::new(x, y, z) (metal_msm.rs:228-241) -- is a projective REPRESENTATIVE of that group
 * element: X : Y : Z depends on the order in which the points of a bucket were added, and the counting sort places the entries of a bucket
 * with LDS atomics, so the 24 words generally DIFFER BETWEEN TWO IDENTICAL CALLS (arkworks compares projectively: `==` on G1Projective
 * holds).  The reference's own sort is serial (shader/cuzk/transpose.metal:8-65), so its limbs repeat; a caller that hashes or memcmp's
 * the Jacobian words must either use out_affine_std or create the context with MSM_FLAG_DETERMINISTIC, which returns the Z = 1
 * representative.  (A deterministic PLACEMENT -- every bucket's run sorted by point index in the fine sort's LDS staging -- was measured in
 * round 5 and is not the default: profiles/NOTES_r5.md.)
 *
 * Threading: a context serialises its own calls with an internal mutex; different contexts are
 * independent.  No caller pointer is retained after a call returns.  Nothing aborts or panics:
 * every failure is a negative status plus msm_last_error().
 */
#ifndef MSM_HIP_H
#define MSM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A consumer must be built against the header of the library it loads: check msm_abi_version() == MSM_HIP_ABI_VERSION once after loading
 * (the Rust shim and the Python binding do) -- msm_timings_t and msm_config_t have grown with the ABI number, and the plain getters write the
 * whole struct of THEIR build.  ABI 7: msm_bn254_g1_combine_flags, msm_get_timings_sized / msm_multi_get_timings_sized, msm_multi_get_clock_stats, msm_set_kernel_timing. */
#define MSM_HIP_ABI_VERSION 7u

/* status codes */
#define MSM_OK 0
#define MSM_ERR_EMPTY (-1)      /* n == 0: reference returns Err("Empty input"), metal_msm.rs:647-649 */
#define MSM_ERR_BAD_ARG (-2)    /* NULL pointer, bad form/flags, scalar >= 2^254, window out of range   */
#define MSM_ERR_NO_DEVICE (-3)  /* no HIP device / extension unusable: the product never falls back to CPU */
#define MSM_ERR_HIP (-4)        /* a HIP runtime call failed; see msm_last_error()                      */
#define MSM_ERR_OOM (-5)
#define MSM_ERR_STATE (-6)      /* e.g. resident call without uploaded bases                            */
#define MSM_ERR_INVALID_DATA (-7) /* a compressed point does not decode (arkworks SerializationError::InvalidData) */
#define MSM_ERR_RCCL (-8)       /* an RCCL call of the multi-GPU exchange failed; see msm_multi_last_error()            */

/* coordinate form of the bases handed in */
#define MSM_FORM_STD 0u  /* plain integers < p   (what pack_affine_and_scalars emits)          */
#define MSM_FORM_MONT 1u /* x*2^256 mod p        (arkworks Fq.0 as is)                          */

/* msm_config_t.flags */
#define MSM_FLAG_UNSIGNED_DIGITS 1u /* plain radix-2^c digits, 2^c-1 buckets/window (BASELINE config "fixed 16-bit window") */
#define MSM_FLAG_NO_GLV 2u          /* do not split scalars with the curve endomorphism (csrc/glv_bn254.hpp); the default splits
                                       k = k1 + lambda*k2, |k_j| < 7*2^123: 2N points phi-extended, half the windows        */

#define MSM_FLAG_WINDOW_TABLE 4u     /* msm_bn254_g1_upload_bases / _upload_compressed also precompute the
                                       WINDOW TABLE of the resident set, T_j[i] = 2^(c*j) P_i for every window j (c doublings and one
                                       inversion per record, once per upload), and msm_bn254_g1_resident / _resident_batch on the whole
                                       set add a digit of window j as +-T_j[i] into ONE bucket array shared by all windows: the buckets are
                                       reduced once per MSM instead of once per window, which moves the optimum to wider windows (c = 20
                                       at 2^20 points: 13 windows instead of 16, 19 % fewer additions, a 19-position host chain instead of
                                       254).  Memory: W x 64 bytes per (virtual) point -- 872 MB at 2^20 -- see msm_plan_t.table_bytes; build 28 ms at
                                       2^20 (what ~300 MSMs gain: for base sets that outlive many calls, e.g. a proving key); none above 2^21.
                                       Every other entry point, and a resident call on fewer scalars than bases, is unaffected.
                                       Results are the same group element either way (bit-exact affine coordinates).            */

#define MSM_FLAG_DETERMINISTIC 8u     /* out_jacobian_mont is the CANONICAL representative of the result: (x*R, y*R, R), the identity (R, R, 0) -- the
                                       same 24 words for the same group element.  Without it the words are A representative that MAY DIFFER
                                       BETWEEN IDENTICAL CALLS (see "Determinism" below).  Costs one field inversion on the host (~10 us;
                                       shared with out_affine_std when both are asked for).  ABI 6.                              */

typedef struct msm_ctx msm_ctx;

typedef struct {
    int32_t device;       /* HIP device ordinal; -1 = current device                                   */
    uint32_t window_bits; /* c; 0 = planner (replaces the N->window table at metal_msm.rs:661-673)     */
    uint32_t flags;       /* MSM_FLAG_*                                                                */
    uint32_t stream_chunk_log2; /* the host-pointer entries cut n >= 2 * 2^this points into chunks of 2^this points: chunk j+1
                                   travels host->HBM (copy stream) while chunk j is sorted and accumulated INTO the shared bucket
                                   array; one bucket reduction and one host finish per MSM (BASELINE config 5).
                                   0 = automatic: from 2^19 points on, uniform chunks of 2^18..2^20 points (a remainder below half a chunk
                                   joins the last one).
                                   Copies run on a stream with a hardware queue of its own: from pinned caller memory at the link
                                   rate, from pageable memory as fast as the runtime stages it (both overlap the kernels) */
    uint64_t max_points;  /* pre-size the HBM workspace for this many points; 0 = grow on demand        */
    uint32_t batch_layout; /* MSM_BATCH_LAYOUT_*: how msm_bn254_g1_resident_batch shares the GPU between its two pipelines (ABI 5) */
    uint32_t host_threads; /* ABI 6 (was `reserved`): CPU threads of the host finish (the Horner chain over the bit sums), the caller included.
                              0 = default (2: the caller + one worker -- every further worker lowers the median by microseconds and raises the
                              mean through 2-8 ms outliers on busy hosts); 1 = the calling thread alone; at most 64 */
} msm_config_t;

/* msm_config_t.batch_layout.  The layout of a batch call is a pure function of (this field, the context's tuned choice, n): nothing
 * is timed behind the caller's back (the reference's whole configuration surface is one struct, metal_msm.rs:16-28).
 *   ONE_STREAM         both pipelines queue whole MSMs on ONE compute stream, MSM after MSM without a gap; uploads and host finishes
 *                      happen beside it.  Needs nothing from HIP's stream -> hardware-queue mapping: the layout that stays within ~12 %
 *                      of its best whatever other contexts and streams the process has created.
 *   ONE_STREAM_REDUCE  the same, and each MSM's bucket reduction runs on a second, high-priority stream beside the next MSM's sort:
 *                      3-6 % faster per MSM from 2^19 points when the three streams get hardware queues of their own -- and 25-50 % SLOWER
 *                      when they do not (three or four other contexts alive: profiles/r3_batch_many_contexts.txt).
 *   TWO_STREAMS        each pipeline keeps its own compute stream and the kernels overlap: best below 2^19 points, where no kernel fills
 *                      the GPU.
 *   AUTO (0)           ONE_STREAM from 2^19 points, TWO_STREAMS below -- unless msm_tune_batch() has measured this context. */
#define MSM_BATCH_LAYOUT_AUTO 0u
#define MSM_BATCH_LAYOUT_ONE_STREAM 1u
#define MSM_BATCH_LAYOUT_ONE_STREAM_REDUCE 2u
#define MSM_BATCH_LAYOUT_TWO_STREAMS 3u

typedef struct {
    uint32_t window_bits;  /* c                                         */
    uint32_t num_windows;  /* W                                         */
    uint32_t num_buckets;  /* buckets per window (2^(c-1) signed, 2^c unsigned incl. an unused slot) */
    uint32_t signed_digits;
    uint64_t workspace_bytes;
    uint64_t virtual_points; /* points each window sorts and accumulates: n, or 2n with the GLV split       */
    uint32_t glv;            /* 1 = scalars are split with the endomorphism                                  */
    uint32_t scalar_bits;    /* bits the windows cover: 254, or 127 with GLV                                 */
    uint32_t table_factor;   /* f: window-table levels per base (MSM_FLAG_WINDOW_TABLE); 1 = no table        */
    uint32_t bucket_arrays;  /* num_windows / table_factor bucket arrays of num_buckets buckets each         */
    uint64_t table_bytes;    /* HBM the window table of the resident set takes (0 without one)               */
    uint32_t top_digit_bits; /* the TOP window's bucket index holds the digit magnitude - 1 in its low top_digit_bits bits; when that is
                                less than log2(num_buckets) -- the top window only holds 254 - c*(W-1) bits (split plans: the halves are
                                below 2^125.81) -- the bits above hold low bits of the point index, so that its buckets are as full as
                                every other window's (csrc/msm_planner.hpp)                                    */
    uint32_t reserved;
} msm_plan_t;

/* per-stage device times of the last call on this context, milliseconds (hipEvent) */
typedef struct {
    float h2d_ms;        /* host->HBM copies (0 for device-resident calls)      */
    float convert_ms;    /* bases to Montgomery / internal layout               */
    float decompose_ms;  /* scalar windowing + signed digits + bucket histogram */
    float sort_ms;       /* bucket offsets (scan) + scatter of point indices    */
    float accumulate_ms; /* per-bucket point accumulation -- the graded kernel  */
    float reduce_ms;     /* bucket reduction (row / column sums, bit sums).  Until ABI 5 this field also held what is now combine_ms */
    float finish_ms;     /* host Horner over the bit sums (+ normalisation if asked) */
    float total_ms;      /* wall clock of the whole call                        */
    uint64_t num_points;
    uint64_t num_adds;   /* mixed additions executed by accumulate (non-zero digits) */
    uint32_t stream_chunks; /* host->HBM chunks the call was cut into (0 = single shot / device-resident)      */
    uint32_t batch_layout;  /* MSM_BATCH_LAYOUT_* the last msm_bn254_g1_resident_batch call of this context ran under (0 before a batch call) */
    float plan_ms;       /* ABI 6: the accumulation's work-item plan (k_piece_count + k_piece_scatter: whole buckets sorted by length), between
                            sort_ms and accumulate_ms -- work the round-3 accumulation kernel did itself                              */
    float combine_ms;    /* ABI 6: k_combine_pieces (buckets cut into pieces), between accumulate_ms and reduce_ms; was counted in reduce_ms */
} msm_timings_t;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* replaces MetalMSMPipeline::with_default_config() (metal_msm.rs:64, rebuilt on EVERY call there) */
int32_t msm_ctx_create(const msm_config_t *cfg /* NULL = defaults */, msm_ctx **out);
void msm_ctx_destroy(msm_ctx *ctx);
/* message of the last failure on ctx (or of the last failed msm_ctx_create when ctx == NULL) */
const char *msm_last_error(const msm_ctx *ctx);
uint32_t msm_abi_version(void);

/* ---- the drop-in call: host pointers in, host results out ----------------------------------
 * Round 6: pageable caller memory is PINNED IN PLACE for the duration of a host-pointer call (hipHostRegister; msm_bn254_g1, _arkworks, _resident(_batch),
 * _upload_bases, the msm_multi forms) and unregistered when the call has consumed it: the copies run at the link rate (53-55 GB/s instead of the ~40 of
 * staged pageable copies -- 2^20 points 2.55 -> 2.45 ms) and registration costs microseconds on this platform.  Memory the caller pinned itself is left alone;
 * a range that cannot be registered travels as before; registrations are reference-counted across contexts and threads of the process. */
/* replaces metal_variable_base_msm (metal_msm.rs:642-695).  bases: n x 16 words; inf_mask: n bytes
 * (non-zero = point at infinity, arkworks G1Affine.infinity) or NULL; scalars: n x 8 words.
 * Any of the three outputs may be NULL.  out_jacobian_mont is the reference's own result type (G::new(x, y, z),
 * metal_msm.rs:228-241): a representative that may differ between identical calls unless the context has MSM_FLAG_DETERMINISTIC.  out_affine_std = canonical affine, standard form (0,0 when the result is the identity and
 * *out_is_inf = 1); it costs the call's only field inversion (~10 us on the host) -- pass NULL to skip it and normalise
 * later with msm_bn254_g1_combine(partial, 1, ...) if needed. */
int32_t msm_bn254_g1(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask,
                     const uint32_t *scalars, size_t n, uint32_t out_jacobian_mont[24],
                     uint32_t out_affine_std[16], uint8_t *out_is_inf);

/* ---- zero-copy arkworks ingestion ------------------------------------------
 * bases: array of n `ark_bn254::G1Affine` structs exactly as they sit in memory, described by (stride, byte offsets of
 * x, y and the `infinity` bool; inf_off = (size_t)-1 if there is none) -- the Rust shim measures these with
 * size_of / addr_of!, the struct is not repr(C).  Coordinates and scalars are arkworks' internal Montgomery words
 * (Fq.0 / Fr.0, R = 2^256): no CPU-side `into_bigint()`, no repacking (replaces pack_affine_and_scalars,
 * utils/limbs_conversion.rs:311-378: 3 Montgomery reductions + 3 heap allocations per point).
 * Round 6: the call first runs as if no struct had its `infinity` flag set (the words are repacked on the device and gathered as they are, the sort
 * overlaps the transfer of the bases); if one does, the call is repeated internally with the flags as an infinity mask -- same result, about twice
 * the time for such inputs (proving keys and SRS points are never at infinity). */
int32_t msm_bn254_g1_arkworks(msm_ctx *ctx, const void *bases, size_t stride, size_t x_off, size_t y_off, size_t inf_off,
                              const uint32_t *scalars_mont, size_t n, uint32_t out_jacobian_mont[24],
                              uint32_t out_affine_std[16], uint8_t *out_is_inf);

/* ---- bases resident in HBM ------------------------------------- */
int32_t msm_bn254_g1_upload_bases(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form,
                                  const uint8_t *inf_mask, size_t n);
int32_t msm_bn254_g1_resident(msm_ctx *ctx, const uint32_t *scalars, size_t n, uint32_t out_jacobian_mont[24],
                              uint32_t out_affine_std[16], uint8_t *out_is_inf);
/* the same with the scalars already in HBM (ABI 4): d_scalars = n x 8 words of device memory, e.g. the witness of a prover whose
 * earlier stages ran on the GPU; hip_stream = the hipStream_t that produced them (NULL = the context's stream).  Nothing crosses
 * PCIe but the 96-byte result, the bases are not converted again (msm_bn254_g1_device converts its bases on every call), and a
 * context created with MSM_FLAG_WINDOW_TABLE uses the table: 2^20 points 1.28 ms against the 1.41 of msm_bn254_g1_device in the same run (1.35 without the table).
 * Blocks until the result is on the host. */
int32_t msm_bn254_g1_resident_device(msm_ctx *ctx, const void *d_scalars, size_t n, void *hip_stream,
                                     uint32_t out_jacobian_mont[24], uint32_t out_affine_std[16], uint8_t *out_is_inf);

/* `count` MSMs against the same resident bases, TWO in flight: scalars[i] = n x 8 words (host), results out_jacobian_mont[i*24..],
 * out_affine_std[i*16..] (nullable), out_is_inf[i] (nullable).  This is how provers call MSM: several scalar vectors per proof against
 * fixed bases.  A second pipeline inside the context (second host thread, own workspace) uploads the next
 * scalar vector and finishes the previous MSM on the CPU while the GPU computes: from 2^19 points both pipelines feed ONE compute
 * stream, MSM after MSM without a gap (each MSM's bucket reduction on a second, high-priority stream beside the next MSM's sort);
 * below, where no kernel fills the GPU, each keeps its own stream and the kernels overlap.  Which of the three layouts a call runs
 * under is decided by msm_config_t.batch_layout (see MSM_BATCH_LAYOUT_*), deterministically; msm_get_timings().batch_layout reports it.
 * n is clamped to the resident set; a window table (MSM_FLAG_WINDOW_TABLE) serves calls on the WHOLE set only.
 * Per MSM, single calls -> batch (round 4): 2^14 0.32 -> 0.21 ms, 2^17 0.50 -> 0.35, 2^20 2.1 -> 1.49, 2^22 7.75 -> 5.80.
 * Results are identical to `count` msm_bn254_g1_resident calls; on an error the first failing code is returned. */
int32_t msm_bn254_g1_resident_batch(msm_ctx *ctx, const uint32_t *const *scalars, size_t n, size_t count,
                                    uint32_t *out_jacobian_mont, uint32_t *out_affine_std, uint8_t *out_is_inf);
/* Explicit, opt-in measurement of the batch layout (ABI 5): runs the batch `scalars[0..count)` (count >= 2; results discarded) under each
 * of the three layouts on THIS context as the process is now -- once untimed (a layout's first use creates hardware queues and the
 * second pipeline's workspace), then `reps` (0 = 3) timed batches, the minimum counts -- and keeps the fastest for this size class
 * (below / from 2^19 points) until the next msm_bn254_g1_upload_bases / _upload_compressed; AUTO then uses it.  *chosen (nullable)
 * receives the layout, ms_per_msm[3] (nullable) the three measurements in the order ONE_STREAM, ONE_STREAM_REDUCE, TWO_STREAMS.
 * A context whose msm_config_t.batch_layout is not AUTO keeps its configured layout (the measurements are still returned). */
int32_t msm_tune_batch(msm_ctx *ctx, const uint32_t *const *scalars, size_t n, size_t count, uint32_t reps, uint32_t *chosen,
                       double *ms_per_msm);

/* ---- arkworks `serialize_compressed` point images ---------------
 * The reference's benchmark harness keeps its instances on disk as `Vec<G1Affine>::serialize_compressed`
 * (mopro-msm/src/msm/utils/preprocess.rs:193-223 writes, 101-131 / 225-256 read): per point 32 bytes = x in
 * standard form, little-endian, with bit 255 = "y is the larger of (y, p-y)" and bit 254 = point at infinity
 * (ark-ec 0.4 SWFlags).  Reading them back costs arkworks one Fq square root per point on the CPU; here the
 * square root y = (x^3+3)^((p+1)/4) runs on the GPU, one thread per point.
 * compressed: n x 32 bytes (host).  An image with both flag bits set, x >= p, or x^3+3 a non-residue fails the
 * whole call with MSM_ERR_INVALID_DATA and *first_invalid (nullable) = the lowest such index.               */
/* decode to arkworks Montgomery words (R = 2^256): out_xy_mont n x 16 words, out_inf n bytes (both host)   */
int32_t msm_bn254_g1_decompress(msm_ctx *ctx, const uint8_t *compressed, size_t n, uint32_t *out_xy_mont,
                                uint8_t *out_inf, int64_t *first_invalid);
/* decode straight into the resident-bases set (then msm_bn254_g1_resident); nothing returns to the host   */
int32_t msm_bn254_g1_upload_compressed(msm_ctx *ctx, const uint8_t *compressed, size_t n, int64_t *first_invalid);
/* the inverse, on the host (no context, no GPU): bases as for msm_bn254_g1 -> n x 32 bytes                */
int32_t msm_bn254_g1_compress(const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask, size_t n,
                              uint8_t *out_compressed);

/* ---- everything already in HBM (what bench.py times) ---------------------------------------- */
/* d_bases_mont: n x 16 words, Montgomery form, device memory; d_inf_mask: n bytes device memory or NULL;
 * d_scalars: n x 8 words device memory.  hip_stream: a hipStream_t (NULL = the context's stream).
 * Blocks until the result is on the host. */
int32_t msm_bn254_g1_device(msm_ctx *ctx, const void *d_bases_mont, const void *d_inf_mask, const void *d_scalars,
                            size_t n, void *hip_stream, uint32_t out_jacobian_mont[24],
                            uint32_t out_affine_std[16], uint8_t *out_is_inf);

/* ---- multi-GPU: fold per-rank partial results (host arithmetic, like final_reduction
 *      metal_msm.rs:204-261 runs on the CPU).  partials: k x 24 words Jacobian Montgomery. -------- */
int32_t msm_bn254_g1_combine(const uint32_t *partials_jacobian_mont, size_t k, uint32_t out_jacobian_mont[24],
                             uint32_t out_affine_std[16], uint8_t *out_is_inf);
/* the same with the representative chosen by the caller (ABI 7): flags = 0 behaves as msm_bn254_g1_combine; MSM_FLAG_DETERMINISTIC hands out the
 * Z = 1 representative, i.e. the words a single context or msm_multi with that flag returns for the same group element -- what a
 * one-process-per-GPU job folds its ranks' partials with when its contexts carry the flag (mopro_msm_hip.distributed.all_reduce_msm).
 * Any other flag bit: MSM_ERR_BAD_ARG. */
int32_t msm_bn254_g1_combine_flags(const uint32_t *partials_jacobian_mont, size_t k, uint32_t flags, uint32_t out_jacobian_mont[24],
                                   uint32_t out_affine_std[16], uint8_t *out_is_inf);

/* ---- BN254 G2 (the Groth16 B query, sum w_i * B2_i): the twist y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1) ------------------
 * The same context, planner and flags as the G1 calls: MSM_FLAG_DETERMINISTIC, MSM_FLAG_NO_GLV (the split uses phi2(x, y) = (beta^2 x, y)),
 * MSM_FLAG_UNSIGNED_DIGITS and window_bits are honoured; a scalar >= 2^254 fails the call with MSM_ERR_BAD_ARG and the context stays usable;
 * msm_get_timings describes the last call.  No window table, resident set or batch form.
 * bases_xy: n x 32 words (x.c0, x.c1, y.c0, y.c1; 8 words each), MSM_FORM_STD or MSM_FORM_MONT (= the words of ark_bn254 Fq2, R = 2^256);
 *   the MSM itself does NOT validate the points: they must lie in G2 (what arkworks' G2Affine guarantees).  msm_bn254_g2_decompress(_device) and
 *   msm_bn254_g2_validate(_device) below give that guarantee on the GPU for bases that come from outside.
 * inf_mask: n bytes or NULL; scalars: n x 8 words, standard form.
 * out_jacobian_mont = X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1 (R = 2^256 Montgomery words; the identity is (1, 1, 0)), out_affine_std = x.c0 x.c1 y.c0 y.c1
 *   in standard form (all zero for the identity); both nullable.  Errors as for msm_bn254_g1: MSM_ERR_EMPTY for n = 0, MSM_ERR_BAD_ARG for a NULL
 *   pointer or a bad form; without a GPU no context exists (msm_ctx_create returns MSM_ERR_NO_DEVICE). */
int32_t msm_bn254_g2(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask,
                     const uint32_t *scalars, size_t n, uint32_t out_jacobian_mont[48],
                     uint32_t out_affine_std[32], uint8_t *out_is_inf);
/* everything in HBM: d_bases_mont n x 32 words Montgomery form, d_inf_mask n bytes or NULL, d_scalars n x 8 words; hip_stream as for
 * msm_bn254_g1_device.  Blocks until the result is on the host. */
int32_t msm_bn254_g2_device(msm_ctx *ctx, const void *d_bases_mont, const void *d_inf_mask, const void *d_scalars,
                            size_t n, void *hip_stream, uint32_t out_jacobian_mont[48],
                            uint32_t out_affine_std[32], uint8_t *out_is_inf);
/* host only, no GPU: fold k partials of 48 words (Jacobian Montgomery, as above) in order; flags 0 or MSM_FLAG_DETERMINISTIC (the Z = 1
 * representative), any other bit MSM_ERR_BAD_ARG; k = 0 MSM_ERR_EMPTY. */
int32_t msm_bn254_g2_combine(const uint32_t *partials_jacobian_mont, size_t k, uint32_t flags,
                             uint32_t out_jacobian_mont[48], uint32_t out_affine_std[32], uint8_t *out_is_inf);

/* ---- getting G2 bases in safely: compressed images, curve and subgroup checks ------------------------------------------------
 * arkworks checks every point when a key is deserialized, on the CPU: one Fq2 square root per compressed point, and one subgroup test per point --
 * the twist's cofactor is 2p - r, not 1, so a point on the twist need not lie in G2.  Here both run on the GPU, one thread per point.
 * Image format (what ark-serialize 0.4 writes for G2Affine::serialize_compressed): 64 bytes = x.c0 then x.c1, each 32 bytes little-endian in
 * standard form; the two flag bits sit in the top bits of byte 63 (the same positions relative to the last coordinate as in the G1 image):
 * bit 7 = y is the larger of (y, -y), bit 6 = the point at infinity.  Fq2 elements are ordered by c1 first, then by c0, each compared as a
 * standard-form integer; an all-zero y counts as not larger.  (No arkworks source or Rust toolchain exists on the build machine: like the G1
 * rule, this one rests on the documented ark-ff 0.4 ordering of quadratic extensions and ark-ec 0.4 SWFlags -- SURVEY.md Appendix C.)
 * An image is INVALID when both flag bits are set, a component is >= p, or x^3 + 3/(9+u) is not a square; with MSM_G2_CHECK_SUBGROUP a point
 * outside G2 is invalid too.  An invalid point fails the whole call with MSM_ERR_INVALID_DATA, *first_invalid (nullable) receives the lowest such
 * index (-1 otherwise) and msm_last_error() says what failed: "decode" (flags, range), "curve" or "subgroup".  The context stays usable.
 * Points flagged infinite (image bit, inf_mask) pass every check; their output coordinates are zero.  n == 0: MSM_ERR_EMPTY.
 * The subgroup test evaluates [x+1]P + psi([x]P) + psi^2([x]P) = psi^3([2x]P) (x the BN parameter, psi the untwist-Frobenius-twist map), which on the
 * twist is equivalent to [r]P = O.  All calls block until the verdict is on the host. */
#define MSM_G2_CHECK_CURVE    1u  /* coordinates < p and y^2 = x^3 + 3/(9+u) */
#define MSM_G2_CHECK_SUBGROUP 2u  /* [r]P = O; implies the curve check */
/* host only, no context, no GPU: bases as for msm_bn254_g2 -> n x 64 bytes.  MSM_ERR_BAD_ARG for a NULL pointer or a bad form. */
int32_t msm_bn254_g2_compress(const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask,
                              size_t n, uint8_t *out_compressed);
/* n x 64 bytes (host) -> n x 32 arkworks Montgomery words + n infinity bytes (host).  The curve check is inherent (the root is verified):
 * checks only adds MSM_G2_CHECK_SUBGROUP; unknown bits MSM_ERR_BAD_ARG.  Pageable caller memory is pinned in place for the copies. */
int32_t msm_bn254_g2_decompress(msm_ctx *ctx, const uint8_t *compressed, size_t n, uint32_t checks,
                                uint32_t *out_xy_mont, uint8_t *out_inf, int64_t *first_invalid);
/* same, results left in caller-owned device memory (n x 128 bytes, 16-byte aligned, and n bytes): exactly what msm_bn254_g2_device takes.  The
 * images are staged in the context's workspace; hip_stream NULL = the context's stream. */
int32_t msm_bn254_g2_decompress_device(msm_ctx *ctx, const uint8_t *compressed, size_t n, uint32_t checks,
                                       void *d_out_xy_mont, void *d_out_inf, void *hip_stream,
                                       int64_t *first_invalid);
/* uncompressed bases (e.g. a snarkjs zkey's Montgomery words): host and device forms.  checks = MSM_G2_CHECK_CURVE, MSM_G2_CHECK_SUBGROUP or
 * both; 0 or an unknown bit: MSM_ERR_BAD_ARG.  Nothing is written but the verdict. */
int32_t msm_bn254_g2_validate(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form,
                              const uint8_t *inf_mask, size_t n, uint32_t checks, int64_t *first_invalid);
int32_t msm_bn254_g2_validate_device(msm_ctx *ctx, const void *d_bases_mont, const void *d_inf_mask,
                                     size_t n, uint32_t checks, void *hip_stream, int64_t *first_invalid);
/* G1's cofactor is 1: coordinates < p and y^2 = x^3 + 3 ("curve") */
int32_t msm_bn254_g1_validate(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form,
                              const uint8_t *inf_mask, size_t n, int64_t *first_invalid);

/* ---- multi-GPU inside ONE process (the reference has no multi-device code: host/gpu.rs:3-5 opens the
 *      system default device).  The caller-facing signature is the same as the single-GPU calls; the point range is cut
 *      into `ndev` contiguous shards, device g pulls ITS OWN shard over its own PCIe link (one host thread + one context
 *      per device), runs the whole single-GPU pipeline on it, and the 96-byte partial group elements are exchanged:
 *        MSM_MULTI_EXCHANGE_RCCL  ncclAllGather of 24 words per rank over RCCL/xGMI (librccl is dlopen'ed: no link-time
 *                                 dependency), every rank folds in rank order, rank 0's bits are returned;
 *        MSM_MULTI_EXCHANGE_HOST  the partials already sit in pinned host memory: the calling thread folds them.
 *      AUTO (ABI 6): when RCCL is possible (librccl loads, ndev > 1, no device listed twice) msm_multi_create MEASURES both exchanges once --
 *      a few calls on identity partials, the same code path the calls take -- and keeps the faster one for the handle's life
 *      (msm_multi_exchange() says which, msm_multi_get_exchange_probe() what was measured); otherwise HOST.  Each rank's partial is in host
 *      memory when its local call returns, so the RCCL round trip is by construction more work than the host fold; rounds 2-4 preferred it
 *      unmeasured.  (One process PER GPU -- torchrun, mopro_msm_hip.distributed -- always exchanges over RCCL.)  The two exchanges fold
 *      the same partials in the same rank order: identical out_affine_std bits either way, and identical out_jacobian_mont for identical
 *      PARTIALS -- which, like every Jacobian result, repeat between calls only under MSM_FLAG_DETERMINISTIC (see "Determinism").  A device may be listed more than once (tests on a 1-GPU box: {0, 0}). ---------- */
#define MSM_MULTI_EXCHANGE_AUTO 0u
#define MSM_MULTI_EXCHANGE_RCCL 1u
#define MSM_MULTI_EXCHANGE_HOST 2u
typedef struct msm_multi msm_multi;
/* devices == NULL: all visible devices (ndev ignored), or the comma-separated list in MSM_HIP_DEVICES.
 * cfg->device is ignored; the other fields apply to every per-device context.  NULL cfg = defaults. */
int32_t msm_multi_create(const int32_t *devices, int32_t ndev, const msm_config_t *cfg, uint32_t exchange, msm_multi **out);
void msm_multi_destroy(msm_multi *m);
const char *msm_multi_last_error(const msm_multi *m); /* m == NULL: last failed msm_multi_create on this thread */
int32_t msm_multi_num_devices(const msm_multi *m);
uint32_t msm_multi_exchange(const msm_multi *m);      /* MSM_MULTI_EXCHANGE_RCCL or _HOST: what the calls really use */
/* what AUTO measured at creation (ABI 6): ms per exchange on identity partials, best of five; both 0 when nothing was probed (an explicit
 * mode, one device, a duplicated device, no librccl).  Either pointer may be NULL. */
int32_t msm_multi_get_exchange_probe(const msm_multi *m, float *rccl_ms, float *host_ms);
/* same arguments and semantics as msm_bn254_g1 / msm_bn254_g1_arkworks, host pointers */
int32_t msm_bn254_g1_multi(msm_multi *m, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask,
                           const uint32_t *scalars, size_t n, uint32_t out_jacobian_mont[24],
                           uint32_t out_affine_std[16], uint8_t *out_is_inf);
int32_t msm_bn254_g1_multi_arkworks(msm_multi *m, const void *bases, size_t stride, size_t x_off, size_t y_off,
                                    size_t inf_off, const uint32_t *scalars_mont, size_t n,
                                    uint32_t out_jacobian_mont[24], uint32_t out_affine_std[16], uint8_t *out_is_inf);
/* shards already resident: d_bases_mont[g] / d_scalars[g] / d_inf_masks[g] (nullable array, nullable entries) are device
 * pointers on device g holding n_per_dev[g] points (as for msm_bn254_g1_device); entries with n_per_dev[g] == 0 are skipped */
int32_t msm_bn254_g1_multi_device(msm_multi *m, const void *const *d_bases_mont, const void *const *d_inf_masks,
                                  const void *const *d_scalars, const size_t *n_per_dev,
                                  uint32_t out_jacobian_mont[24], uint32_t out_affine_std[16], uint8_t *out_is_inf);
/* timings of device g's part of the last call */
int32_t msm_multi_get_timings(const msm_multi *m, int32_t g, msm_timings_t *out);
/* what the exchange cost in the last call: *exchange_ms = rank 0's wall clock from the end of its local MSM to the folded result
 * (RCCL: the rendezvous with the slowest rank, 96 B up, ncclAllGather, 96*ndev B down, fold; host fold: the fold alone);
 * shard_ms[0..nshard) = wall clock of every rank's local MSM.  Either pointer may be NULL.
 * Error behaviour of the multi calls: a rank whose local MSM fails never leaves its peers waiting in the collective -- the ranks
 * rendezvous on the host first and ALL skip the exchange; the call returns the first failing rank's status, and
 * msm_multi_last_error() names the device and rank (metal_msm.rs:647-656: errors are returned, nothing hangs). */
int32_t msm_multi_get_exchange_stats(const msm_multi *m, float *exchange_ms, float *shard_ms, int32_t nshard);
int32_t msm_multi_get_timings_sized(const msm_multi *m, int32_t rank, void *out, size_t out_size); /* ABI 7, see msm_get_timings_sized */
int32_t msm_multi_set_kernel_timing(msm_multi *m, uint32_t every_n); /* ABI 7: msm_set_kernel_timing on every rank's context */
/* msm_get_clock_stats of rank `rank`'s context (ABI 7): a slow rank of a multi-GPU call can be told from a slow CLOCK on its device */
int32_t msm_multi_get_clock_stats(msm_multi *m, int32_t rank, double *sclk_ghz, double *cycles_per_addition, uint64_t *samples);

/* ---- BN254 scalar field Fr: number-theoretic transforms in HBM (the H scalars of a Groth16 proof, made where the MSM reads them).
 *      Elements are 8 little-endian 32-bit words, as the scalars of the MSM calls.  Added under ABI 7, as the G2 calls were.
 *      Root: w_28 = 5^((r-1)/2^28) mod r = 19103219067921713944291392827692070036145651957329286315305642004821462161904 (arkworks'
 *      Fr::TWO_ADIC_ROOT_OF_UNITY, snarkjs' root), w_k = w_28^(2^(28-k)).  halo2's 7-based root differs from k = 5 on and is NOT offered.
 *      Forward:  A[j] = sum_i a[i] (g w^j)^i, g = 1 without a coset.  Inverse: the exact inverse of that, 1/n included, times g^-i after the
 *      transform when a coset is given.  The generator is an ARGUMENT: arkworks' coset_fft uses g = 5, snarkjs' odd coset g = w_(k+1).
 *      Any 256-bit input pattern is read modulo r; outputs are canonical (< r): results are bit-exact.  log_n == 0 converts the form only.
 *      Errors: log_n > 28, an unknown flag bit, a NULL pointer, g = 0 (mod r), an array not aligned to 16 bytes: MSM_ERR_BAD_ARG; batch == 0
 *      (n == 0): MSM_ERR_EMPTY; allocation failure: MSM_ERR_OOM.  The context stays usable after any of them. ---------------------------- */
#define MSM_NTT_INVERSE  1u  /* inverse transform, 1/n included */
#define MSM_NTT_IN_MONT  2u  /* input words are arkworks Fr.0 (x*2^256 mod r); default: standard form */
#define MSM_NTT_OUT_MONT 4u  /* output words likewise; default: standard form = what the MSM calls take as scalars */
/* host only, no context: the primitive 2^log_n-th root the transforms use, standard form */
int32_t msm_bn254_fr_root_of_unity(uint32_t log_n, uint32_t out_std[8]);
/* host only: how a transform of this size is cut into passes over global memory (radix_log2[i] bits in pass i; the array is read and written
 * once per pass, and there is no separate reordering pass) */
int32_t msm_bn254_fr_ntt_plan(uint32_t log_n, uint32_t *passes, uint32_t radix_log2[8]);
/* in place on `batch` contiguous arrays of n = 2^log_n elements in device memory, natural order in AND out.
 * coset_gen_std: NULL, or a HOST pointer to 8 words g != 0 (standard form).
 * Stream-ordered on hip_stream (NULL = the context's stream): returns when enqueued.  The first use of a size (or of a generator) on a context
 * builds its tables on the same stream first.  A context's calls share one scratch array: a call on another stream than the one before it
 * waits for that one. */
int32_t msm_bn254_fr_ntt_device(msm_ctx *ctx, void *d_data, uint32_t log_n, size_t batch, uint32_t flags,
                                const uint32_t *coset_gen_std, void *hip_stream);
/* host pointers, blocking; out == in allowed; pageable memory is pinned in place like every host-pointer call */
int32_t msm_bn254_fr_ntt(msm_ctx *ctx, const uint32_t *in, uint32_t *out, uint32_t log_n, size_t batch, uint32_t flags,
                         const uint32_t *coset_gen_std);
/* out[i] = (a[i]*b[i] - c[i]) * k.  d_c NULL = no subtrahend.  k_std (host, 8 words) NULL = 1.  d_out may alias any input.
 * flags: MSM_NTT_IN_MONT / MSM_NTT_OUT_MONT only.  Stream-ordered like the transform. */
int32_t msm_bn254_fr_mul_sub_scale_device(msm_ctx *ctx, const void *d_a, const void *d_b, const void *d_c,
                                          const uint32_t *k_std, void *d_out, size_t n, uint32_t flags, void *hip_stream);

/* ---- BN254 scalar field Fr: rows of R1CS constraint matrices times the witness, in HBM (where the evaluations [a | b | c] the H recipes start
 *      from come from: a = A w, b = B w, c = C w or c = a o b).  The matrices stay resident with the key, as the bases do; the witness is the
 *      scalar vector of the A, B1, B2 and L query MSMs and is in HBM already.  Added under ABI 7, as the transforms were.
 *      A record has the layout of one entry of a snarkjs zkey's coefficient section (section 4): matrix, constraint, signal, 32 little-endian
 *      bytes -- the section's payload after its count can be handed over as it is, with MSM_R1CS_COEF_MONT2.  Any 256-bit value pattern is read
 *      modulo r; entries may come in any order; repeated (matrix, row, col) entries add up (each counts as an entry of its row). ---------------- */
#define MSM_R1CS_COEF_STD   0u  /* value = coefficient, plain integer                           */
#define MSM_R1CS_COEF_MONT  1u  /* value = coefficient * 2^256 mod r  (arkworks Fr.0)           */
#define MSM_R1CS_COEF_MONT2 2u  /* value = coefficient * 2^512 mod r  (section 4 of a snarkjs zkey) */
#define MSM_R1CS_C_FROM_AB  8u  /* eval flag: c[i] = a[i]*b[i]; without it c = (matrix 2)*w     */

typedef struct { uint32_t matrix, row, col; uint32_t value[8]; } msm_r1cs_coef_t;  /* 44 bytes, no padding */

/* what an upload builds.  Rows are cut into work items of at most max_item_len <= 24 entries, one GPU lane each (24 additions of a raw 256-bit
 * word or of 7r minus one stay below the 2^261 the lazily reduced sum can hold); a row of several items has its partial sums folded by a second
 * launch.  A row without entries, in a matrix that has any, is a work item of length 0. */
typedef struct {
    uint64_t entries[3];           /* per matrix                                                     */
    uint64_t rows_with_entries[3];
    uint64_t longest_row;          /* entries                                                        */
    uint64_t plus_one, minus_one;  /* entries whose coefficient is 1 / r - 1 (modulo r): no multiplication */
    uint64_t distinct_values;      /* the other coefficients' dictionary                             */
    uint64_t work_items, max_item_len;
    uint64_t fold_rows;            /* rows of more than one item ...                                 */
    uint64_t partial_sums;         /* ... and their items                                            */
    uint64_t device_bytes;
    double build_ms;               /* host: validation, the counting sort by (matrix, row), the dictionary, the layout */
    double upload_ms;              /* the whole upload call, build_ms included (0 from msm_bn254_fr_r1cs_plan)          */
} msm_r1cs_info_t;

/* host only, no context, no GPU: validates the list as the upload does (same errors; the message, msm_last_error(NULL), names the first offending
 * entry) and reports what an upload would build.  The coefficient values are taken as MSM_R1CS_COEF_STD. */
int32_t msm_bn254_fr_r1cs_plan(const msm_r1cs_coef_t *coefs, size_t n_coefs, uint32_t num_rows, uint32_t num_cols, uint32_t log_n,
                               msm_r1cs_info_t *out);
/* builds the resident form of up to three matrices (matrix 0, 1, 2 = A, B, C) of num_rows x num_cols on the context, replacing an earlier one;
 * blocks until it is resident.  The evaluations are laid out over a domain of 2^log_n >= num_rows rows.
 * Errors: n_coefs == 0: MSM_ERR_EMPTY; matrix > 2, row >= num_rows, col >= num_cols, num_rows > 2^log_n, log_n > 28, a bad form:
 * MSM_ERR_BAD_ARG.  After an error the context stays usable and keeps what it held. */
int32_t msm_bn254_fr_r1cs_upload(msm_ctx *ctx, const msm_r1cs_coef_t *coefs, size_t n_coefs, uint32_t coef_form, uint32_t num_rows,
                                 uint32_t num_cols, uint32_t log_n);
/* what the context's latest upload built and how long it took; MSM_ERR_STATE without one */
int32_t msm_bn254_fr_r1cs_info(msm_ctx *ctx, msm_r1cs_info_t *out);
/* d_witness: n_witness = num_cols elements of 8 words; d_out: 3 x 2^log_n elements, written as [a | b | c] -- every row at or above num_rows and
 * every row without entries as zero.  Both in device memory, 16-byte aligned.  flags: MSM_NTT_IN_MONT (the witness words are w*2^256),
 * MSM_NTT_OUT_MONT (the output words likewise), MSM_R1CS_C_FROM_AB.  Outputs are canonical (< r).
 * Stream-ordered on hip_stream (NULL = the context's stream): returns when enqueued.  Rows of more than 24 entries go through a per-context
 * array of partial sums: an eval on another stream than the one before it waits for that one.
 * Errors: no upload: MSM_ERR_STATE; n_witness != num_cols, an unknown flag bit, a NULL or misaligned pointer: MSM_ERR_BAD_ARG. */
int32_t msm_bn254_fr_r1cs_eval_device(msm_ctx *ctx, const void *d_witness, size_t n_witness, void *d_out, uint32_t flags, void *hip_stream);
/* host pointers, blocking; pageable memory is pinned in place like every host-pointer call */
int32_t msm_bn254_fr_r1cs_eval(msm_ctx *ctx, const uint32_t *witness, size_t n_witness, uint32_t *out, uint32_t flags);

/* ---- BN254 G1 fixed-base batch multiplication (ABI 7): out[i] = k_i * P, one base, n scalars, n affine points -- the shape of
 *      arkworks' FixedBase::msm / batch_mul: the A, B1, L and H queries of a Groth16 setup, the powers of a KZG setup.
 *      A scalar is ANY 256-bit pattern, read as an integer: k * P is (k mod r) * P, as the transforms and the R1CS rows read their inputs.  There is
 *      no range check and nothing comes back from the device, so the device form is stream-ordered.  With MSM_NTT_IN_MONT the words are arkworks
 *      Fr.0 (k * 2^256 mod r) and one multiplication by a constant brings them to canonical standard form first.
 *      Output coordinates are canonical (< p): results are bit-exact.  k_i * P = the identity: out_inf[i] = 1 and all sixteen words zero.
 *      The base is checked on the host: coordinates < p and y^2 = x^3 + 3, else MSM_ERR_INVALID_DATA.
 *      The window table of (base, window_bits) -- W * 2^(c-1) affine records of 64 bytes, 2.9 MB at the default c = 12, 270 KB at c = 8 -- is built on the device, on the call's
 *      stream, and kept on the context; it is rebuilt only when the base (compared after normalising its form) or c changes.  Table and events are
 *      per context: a call on another stream than the one before it waits for that one.  The inv_group points of a workgroup share ONE field
 *      inversion (Montgomery's trick in the workgroup's LDS): no scratch array in HBM exists, and a call of any n is cut into launches of at most
 *      2^30 points.  The host-pointer form stages at most 2^20 points (97 MB of device memory) at a time.
 *      Errors: base off the curve or a coordinate >= p: MSM_ERR_INVALID_DATA; n == 0: MSM_ERR_EMPTY; a NULL or misaligned pointer, a bad form, an
 *      unknown flag bit, window_bits not 0 or 4..16: MSM_ERR_BAD_ARG; allocation failure: MSM_ERR_OOM.  The context stays usable after any. ---- */
#define MSM_FB_OUT_STD 8u   /* output coordinates in standard form; default: arkworks Montgomery words (what msm_bn254_g1_device /
                               _upload_bases(MSM_FORM_MONT) take) */
/* MSM_NTT_IN_MONT (2u) is honoured too: scalar words are arkworks Fr.0 (k*2^256 mod r) */

typedef struct {
    uint32_t window_bits;   /* c */
    uint32_t num_windows;   /* W = ceil(257 / c): signed digits of a 256-bit integer may carry one bit out */
    uint64_t table_entries; /* W * 2^(c-1) */
    uint64_t table_bytes;
    uint32_t inv_group;     /* points that share one field inversion */
    uint32_t reserved;
} msm_fixed_base_plan_t;

/* host only, no context: window_bits 0 = the default; 4..16 otherwise, anything else MSM_ERR_BAD_ARG */
int32_t msm_bn254_g1_fixed_base_plan(uint32_t window_bits, msm_fixed_base_plan_t *out);

/* out[i] = k_i * P.  base_xy: HOST pointer, 16 words (x, y), base_form MSM_FORM_STD / _MONT; d_scalars: n x 8 words;
 * d_out_xy: n x 16 words; d_out_inf: n bytes (1 = k_i * P is the identity, coordinates all zero) -- device memory, 16-byte aligned.
 * Stream-ordered on hip_stream (NULL = the context's stream): returns when enqueued.  Blocking host-pointer form below. */
int32_t msm_bn254_g1_fixed_base_mul_device(msm_ctx *ctx, const uint32_t *base_xy, uint32_t base_form, const void *d_scalars, size_t n,
                                           uint32_t window_bits, uint32_t flags, void *d_out_xy, void *d_out_inf, void *hip_stream);
int32_t msm_bn254_g1_fixed_base_mul(msm_ctx *ctx, const uint32_t *base_xy, uint32_t base_form, const uint32_t *scalars, size_t n,
                                    uint32_t window_bits, uint32_t flags, uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 G2 fixed-base batch multiplication (ABI 7): out[i] = k_i * Q for one base Q of G2, n scalars, n affine points of
 *      32 words (x.c0, x.c1, y.c0, y.c1) -- the B2 query of a Groth16 setup (k_i * H), the G2 powers of a KZG setup.  Scalars, flags
 *      (MSM_NTT_IN_MONT, MSM_FB_OUT_STD), output forms, the infinity bytes (k_i = 0 mod r: out_inf[i] = 1 and all 32 words zero) and the
 *      errors are those of the G1 call above; the outputs are what msm_bn254_g2_device takes as d_bases_mont / d_inf_mask.
 *      The base is checked on the host every call: components < p and y^2 = x^3 + 3/(9+u) ("curve" in msm_last_error), and, whenever it is not
 *      the base the context's table was built from, [r]Q = O ("subgroup") -- the twist's cofactor is not 1, and reading a 256-bit scalar as
 *      (k mod r) is only right in G2.  Either failure: MSM_ERR_INVALID_DATA, and the table of the previous base stays in place.
 *      The window table of (base, window_bits) -- W * 2^(c-1) affine records of 128 bytes, 5.8 MB at the default c = 12 -- is built on the device,
 *      on the call's stream, and kept on the context beside (not instead of) the G1 call's table; it is rebuilt only when the base (compared as
 *      Montgomery words) or c changes.  The products of a chunk of chunk_points scalars go through a per-context array of XYZZ records
 *      (scratch_bytes) and are normalised by a second kernel in which every lane inverts a chain of inv_group points with ONE field inversion;
 *      a call of any n is cut into such chunks.  Table, scratch array and event are per context: a call on another stream than the one before
 *      it waits for that one.  The host-pointer form stages chunk_points points (42 MB of device memory) at a time. ---- */
typedef struct {
    uint32_t window_bits;   /* c */
    uint32_t num_windows;   /* W = ceil(257 / c) */
    uint64_t table_entries; /* W * 2^(c-1) */
    uint64_t table_bytes;   /* records of 128 bytes */
    uint32_t inv_group;     /* points that share one field inversion */
    uint32_t chunk_points;  /* points per pass through the scratch array (device form) and per staging step (host form) */
    uint64_t scratch_bytes; /* the per-context XYZZ scratch array of one chunk */
} msm_fixed_base_g2_plan_t;

/* host only, no context: window_bits 0 = the default; 4..16 otherwise, anything else MSM_ERR_BAD_ARG */
int32_t msm_bn254_g2_fixed_base_plan(uint32_t window_bits, msm_fixed_base_g2_plan_t *out);

/* out[i] = k_i * Q.  base_xy: HOST pointer, 32 words, base_form MSM_FORM_STD / _MONT; d_scalars: n x 8 words; d_out_xy: n x 32 words;
 * d_out_inf: n bytes -- device memory, 16-byte aligned.  Stream-ordered on hip_stream (NULL = the context's stream): returns when enqueued.
 * Blocking host-pointer form below. */
int32_t msm_bn254_g2_fixed_base_mul_device(msm_ctx *ctx, const uint32_t *base_xy, uint32_t base_form, const void *d_scalars, size_t n,
                                           uint32_t window_bits, uint32_t flags, void *d_out_xy, void *d_out_inf, void *hip_stream);
int32_t msm_bn254_g2_fixed_base_mul(msm_ctx *ctx, const uint32_t *base_xy, uint32_t base_form, const uint32_t *scalars, size_t n,
                                    uint32_t window_bits, uint32_t flags, uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 G1 element-wise scalar multiplication (ABI 7): out[i] = k_i * P_i -- n DIFFERENT points, each multiplied by a
 *      scalar of its own (or all by one scalar), n affine points out.  What an update of an existing setup consists of: a powers-of-tau
 *      contribution (tauG1[i] <- tau'^i * tauG1[i]), a Groth16 phase-2 contribution (every L and H point times 1/delta'), a re-randomised base
 *      set.  Where the points share one base, the fixed-base call above is the call to use (its table makes it many times faster).
 *      The fixed-base calls' contract holds wherever it applies.  Scalars: 8 little-endian words, ANY 256-bit pattern, read modulo r; with
 *      MSM_NTT_IN_MONT the words are arkworks Fr.0 (k*2^256 mod r).  Bases: n x 16 words (x, y) as msm_bn254_g1_device takes them -- arkworks
 *      Montgomery words, standard-form integers with MSM_PM_BASES_STD -- and n bytes d_inf_mask (nonzero = the point at infinity, its words
 *      ignored) or NULL.  The bases must be curve points with coordinates below p; the call does NOT validate them (msm_bn254_g1_validate does):
 *      words that are no curve point give a meaningless point at their place, never a fault and never a wrong neighbour -- the kernel makes no
 *      data-dependent memory access.  Outputs: canonical coordinates, Montgomery words by default, standard form with MSM_FB_OUT_STD;
 *      out_inf[i] = 1 and all sixteen words zero for the identity (the base is flagged, or k_i = 0 mod r), out_inf[i] = 0 otherwise.
 *      Aliasing: d_out_xy == d_bases_xy and d_out_inf == d_inf_mask are allowed (each on its own) -- a ceremony updates in place; any other
 *      overlap between the arrays of a call is the caller's error.
 *      The device forms are stream-ordered on hip_stream (NULL = the context's stream) and return when enqueued.  Like the msm_bn254_fr_*_device
 *      vector calls they keep NOTHING on the context -- no table, no scratch array, no event -- so two calls on two streams do not wait for each
 *      other, and the caller orders calls that share an array.  The inv_group points of a workgroup share two field inversions; a call of any n is
 *      cut into launches of at most 2^30 points.  The host-pointer form stages at most 2^20 points (97 MB of device memory, kept on the context
 *      and released with it) at a time and pins pageable memory like every host-pointer call.
 *      Errors: a NULL pointer (d_inf_mask / inf_mask excepted) or a device array that is not 16-byte aligned, an unknown flag bit, a bad
 *      base_form: MSM_ERR_BAD_ARG; n == 0: MSM_ERR_EMPTY; allocation failure: MSM_ERR_OOM.  The context stays usable after any, and a failed
 *      call writes nothing. ---- */
#define MSM_PM_BASES_STD 16u  /* the base coordinates are standard-form integers; default: arkworks Montgomery words */
/* also honoured: MSM_NTT_IN_MONT (2u; scalar words are Fr.0) and MSM_FB_OUT_STD (8u) */

typedef struct {
    uint32_t inv_group;    /* points that share one field inversion (twice per call: the table's slopes, the outputs) */
    uint32_t ladder_bits;  /* positions of the joint double-and-add ladder: the bits of a half of the GLV split */
    uint32_t table_points; /* affine points a lane keeps in registers: P, lambda * P and their sum, signs folded in */
    uint32_t reserved;
} msm_pointwise_plan_t;

/* host only, no context */
int32_t msm_bn254_g1_pointwise_mul_plan(msm_pointwise_plan_t *out);

/* out[i] = k_i * P_i.  d_bases_xy: n x 16 words; d_inf_mask: n bytes or NULL; d_scalars: n x 8 words; d_out_xy: n x 16 words; d_out_inf: n bytes --
 * device memory, 16-byte aligned.  flags: MSM_NTT_IN_MONT, MSM_FB_OUT_STD, MSM_PM_BASES_STD. */
int32_t msm_bn254_g1_pointwise_mul_device(msm_ctx *ctx, const void *d_bases_xy, const void *d_inf_mask, const void *d_scalars, size_t n,
                                          uint32_t flags, void *d_out_xy, void *d_out_inf, void *hip_stream);
/* out[i] = k * P_i for ONE scalar.  k_std: HOST pointer to 8 standard-form words (any pattern, read modulo r); it is split on the host and
 * travels with the launch, so every lane walks the same ladder.  flags: MSM_FB_OUT_STD, MSM_PM_BASES_STD; MSM_NTT_IN_MONT is MSM_ERR_BAD_ARG. */
int32_t msm_bn254_g1_scale_device(msm_ctx *ctx, const void *d_bases_xy, const void *d_inf_mask, const uint32_t *k_std, size_t n, uint32_t flags,
                                  void *d_out_xy, void *d_out_inf, void *hip_stream);
/* the first one on host pointers, blocking.  base_form: MSM_FORM_STD / _MONT as in msm_bn254_g1 (MSM_PM_BASES_STD is not taken here);
 * inf_mask NULL: no point is flagged; out_xy may be bases_xy and out_inf may be inf_mask. */
int32_t msm_bn254_g1_pointwise_mul(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask, const uint32_t *scalars,
                                   size_t n, uint32_t flags, uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 G1 group transform (ABI 7): the discrete Fourier transform over G1 POINTS, in place, natural order in and out,
 *      with the domain and the direction conventions of msm_bn254_fr_ntt_device:
 *          forward:  out[j] = sum_i w^(ij) * in[i];     with MSM_NTT_INVERSE:  out[i] = n^-1 * sum_j w^(-ij) * in[j]
 *      w = msm_bn254_fr_root_of_unity(log_n), n = 2^log_n.  The inverse turns a powers-of-tau output tauG1[j] = tau^j * G into the Lagrange basis
 *      L_i(tau) * G without anybody knowing tau (snarkjs "powersoftau prepare phase2", halo2's g_lagrange); with tau in hand
 *      msm_bn254_fr_lagrange_device and the fixed-base call are the cheaper route.  (n / 2) * log_n scalar multiplications of points: a
 *      bit-reversal sweep, then log_n radix-2 stages of one lane per butterfly, each the ladder of the element-wise multiplication above, two
 *      complete additions and one normalisation; the first stage (every twiddle 1) runs no ladder.
 *      d_xy: batch contiguous arrays of n x 16 words, the (x, y) records of msm_bn254_g1_pointwise_mul_device; d_inf: batch * n bytes (nonzero =
 *      the point at infinity, its words ignored), REQUIRED: an output can be the identity where no input was.  Both device memory, 16-byte
 *      aligned, read and written.  flags: MSM_NTT_INVERSE (1u), MSM_PM_BASES_STD (16u; the input coordinates are standard-form integers),
 *      MSM_FB_OUT_STD (8u; standard-form output); any other bit is MSM_ERR_BAD_ARG.  Outputs: canonical coordinates, word-exact; the identity is
 *      inf = 1 with sixteen zero words, every other place has inf = 0.  Inputs are NOT validated: words that are no curve point give meaningless
 *      points, never a fault -- the kernels make no data-dependent memory access.  log_n == 0 only converts the form and canonicalises the flag.
 *      Stream-ordered on hip_stream (NULL = the context's stream): the call returns when enqueued.  Kept on the context, per log_n >= 2: the
 *      n / 2 powers of w in standard form (msm_g1_fft_plan_t.table_bytes; one table serves both directions), built on the call's stream by its
 *      first use.  A call on ANOTHER stream waits for the event behind that build, so calls of a context on two streams that first build a
 *      table order themselves; afterwards they do not wait for each other, and the caller orders calls that share an array.
 *      A coset form is not offered: multiply by g^i with msm_bn254_g1_pointwise_mul_device.  The G2 sibling is
 *      msm_bn254_g2_fft_device below; it shares this call's twiddle tables.
 *      Errors: a NULL or misaligned pointer, an unknown flag bit, log_n > 28, batch * n > 2^36, a bad base_form: MSM_ERR_BAD_ARG; batch == 0:
 *      MSM_ERR_EMPTY; allocation failure: MSM_ERR_OOM.  A failed call writes nothing and the context stays usable. ---- */
typedef struct {
    uint16_t stages;         /* butterfly launches per 2^30 butterflies: log_n */
    uint16_t ladder_stages;  /* ... of them with a scalar multiplication per butterfly: log_n - 1 (0 for log_n == 0) */
    uint32_t inv_group;      /* butterflies that share one field inversion (twice per ladder stage: the slopes, the 2 * inv_group outputs) */
    uint64_t table_bytes;    /* kept on the context for this size: n / 2 twiddles of 32 bytes (0 below log_n = 2) */
} msm_g1_fft_plan_t;

/* host only, no context */
int32_t msm_bn254_g1_fft_plan(uint32_t log_n, msm_g1_fft_plan_t *out);
int32_t msm_bn254_g1_fft_device(msm_ctx *ctx, void *d_xy, void *d_inf, uint32_t log_n, size_t batch, uint32_t flags, void *hip_stream);
/* on host pointers, blocking.  base_form: MSM_FORM_STD / _MONT (MSM_PM_BASES_STD is not taken here); inf NULL: nothing is flagged; out_xy may be
 * xy and out_inf may be inf.  The whole batch is staged in device memory (65 bytes per point, kept on the context): a transform cannot be
 * chunked.  Pageable memory is pinned in place like every host-pointer call. */
int32_t msm_bn254_g1_fft(msm_ctx *ctx, const uint32_t *xy, uint32_t base_form, const uint8_t *inf, uint32_t log_n, size_t batch, uint32_t flags,
                         uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 G2 element-wise scalar multiplication (ABI 7): out[i] = k_i * Q_i on G2 records -- the other half of a ceremony
 *      update: the tauG2 section (tauG2[i] <- tau'^i * tauG2[i]) and betaG2 of a powers-of-tau contribution, deltaG2 of a Groth16 phase-2
 *      contribution, a re-randomised G2 base set.  Where the points share one base, msm_bn254_g2_fixed_base_mul_device is the call to use.
 *      The contract is that of the G1 element-wise calls above, word for word, wherever it applies.  Records: a point is 32 words, x.c0, x.c1,
 *      y.c0, y.c1 -- what msm_bn254_g2_device takes as d_bases_mont and msm_bn254_g2_fixed_base_mul_device writes: arkworks Montgomery words,
 *      standard-form integers with MSM_PM_BASES_STD -- and n bytes d_inf_mask (nonzero = the point at infinity, its words ignored) or NULL.
 *      Scalars: 8 little-endian words, ANY 256-bit pattern, read modulo r; with MSM_NTT_IN_MONT the words are arkworks Fr.0.
 *      THE BASES MUST BE POINTS OF G2, the subgroup of order r: the twist's cofactor is not 1, and reading a scalar modulo r is only right in
 *      G2 -- and so is the endomorphism the kernel uses.  The call does NOT validate them; msm_bn254_g2_validate(_device) with
 *      MSM_G2_CHECK_SUBGROUP does.  Anything else -- words that are no curve point, components of p or above, a point of the twist outside
 *      G2 -- gives a meaningless point at its own place, never a fault and never a wrong neighbour: the kernel makes no data-dependent memory
 *      access.  Outputs: canonical components, Montgomery words by default, standard form with MSM_FB_OUT_STD; out_inf[i] = 1 and all 32 words
 *      zero for the identity (the base is flagged, or k_i = 0 mod r), out_inf[i] = 0 otherwise.
 *      Aliasing: d_out_xy == d_bases_xy and d_out_inf == d_inf_mask are allowed (each on its own); any other overlap is the caller's error.
 *      The device forms are stream-ordered on hip_stream (NULL = the context's stream), return when enqueued and keep NOTHING on the context --
 *      no table, no scratch array, no event -- so two calls on two streams do not wait for each other, and the caller orders calls that share an
 *      array.  One kernel per launch: the inv_group points of a workgroup share two field inversions (of the norms, in Fq); a call of any n is
 *      cut into launches of at most 2^30 points.  The host-pointer form stages at most 2^19 points (161 bytes each: 85 MB of device memory,
 *      kept on the context and released with it) at a time and pins pageable memory like every host-pointer call.
 *      Errors, as for G1: a NULL pointer (d_inf_mask / inf_mask excepted) or a device array that is not 16-byte aligned, an unknown flag bit, a
 *      bad base_form: MSM_ERR_BAD_ARG; n == 0: MSM_ERR_EMPTY; allocation failure: MSM_ERR_OOM.  The context stays usable after any, and a
 *      failed call writes nothing. ---- */
typedef struct {
    uint32_t inv_group;    /* points that share one field inversion (twice per call: the table's slopes, the outputs) */
    uint32_t ladder_bits;  /* positions of the joint double-and-add ladder: the bits of a half of the GLV split */
    uint32_t table_points; /* affine points a lane works from: Q, lambda * Q and their sum, signs folded in */
    uint32_t reserved;
} msm_pointwise_g2_plan_t;

/* host only, no context */
int32_t msm_bn254_g2_pointwise_mul_plan(msm_pointwise_g2_plan_t *out);

/* out[i] = k_i * Q_i.  d_bases_xy: n x 32 words; d_inf_mask: n bytes or NULL; d_scalars: n x 8 words; d_out_xy: n x 32 words; d_out_inf: n bytes --
 * device memory, 16-byte aligned.  flags: MSM_NTT_IN_MONT, MSM_FB_OUT_STD, MSM_PM_BASES_STD. */
int32_t msm_bn254_g2_pointwise_mul_device(msm_ctx *ctx, const void *d_bases_xy, const void *d_inf_mask, const void *d_scalars, size_t n,
                                          uint32_t flags, void *d_out_xy, void *d_out_inf, void *hip_stream);
/* out[i] = k * Q_i for ONE scalar.  k_std: HOST pointer to 8 standard-form words (any pattern, read modulo r); it is split on the host and
 * travels with the launch, so every lane walks the same ladder.  flags: MSM_FB_OUT_STD, MSM_PM_BASES_STD; MSM_NTT_IN_MONT is MSM_ERR_BAD_ARG. */
int32_t msm_bn254_g2_scale_device(msm_ctx *ctx, const void *d_bases_xy, const void *d_inf_mask, const uint32_t *k_std, size_t n, uint32_t flags,
                                  void *d_out_xy, void *d_out_inf, void *hip_stream);
/* the first one on host pointers, blocking.  base_form: MSM_FORM_STD / _MONT as in msm_bn254_g2 (MSM_PM_BASES_STD is not taken here);
 * inf_mask NULL: no point is flagged; out_xy may be bases_xy and out_inf may be inf_mask. */
int32_t msm_bn254_g2_pointwise_mul(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask, const uint32_t *scalars,
                                   size_t n, uint32_t flags, uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 G2 group transform (ABI 7): the discrete Fourier transform over G2 POINTS, in place, natural order in and out
 *      -- the G1 group transform above on the records of the G2 element-wise calls, with its contract word for word:
 *          forward:  out[j] = sum_i w^(ij) * in[i];     with MSM_NTT_INVERSE:  out[i] = n^-1 * sum_j w^(-ij) * in[j]
 *      w = msm_bn254_fr_root_of_unity(log_n), n = 2^log_n.  The inverse turns the tauG2 section tauG2[j] = tau^j * H of a powers-of-tau file into
 *      L_i(tau) * H without anybody knowing tau (the G2 half of snarkjs "powersoftau prepare phase2").  A bit-reversal sweep, then log_n radix-2
 *      stages of one lane per butterfly, each the ladder of the G2 element-wise multiplication, two complete additions and one normalisation
 *      through the norms; the first stage (every twiddle 1) runs no ladder; no scratch array.
 *      d_xy: batch contiguous arrays of n x 32 words (x.c0 x.c1 y.c0 y.c1, the records of msm_bn254_g2_pointwise_mul_device); d_inf: batch * n
 *      bytes (nonzero = the point at infinity, its words ignored), REQUIRED.  Both device memory, 16-byte aligned, read and written.  flags:
 *      MSM_NTT_INVERSE (1u), MSM_PM_BASES_STD (16u), MSM_FB_OUT_STD (8u); any other bit is MSM_ERR_BAD_ARG.  Outputs: canonical components,
 *      word-exact; the identity is inf = 1 with 32 zero words, every other place has inf = 0.  log_n == 0 only converts the form and
 *      canonicalises the flag.  log_n <= 28 and batch * n <= 2^36.
 *      THE INPUTS MUST BE POINTS OF G2, the subgroup of order r, not only of the twist: the twist's cofactor is not 1, and reading a twiddle
 *      modulo r and the endomorphism of the ladder are only right in G2.  The call does NOT validate them; msm_bn254_g2_validate(_device) with
 *      MSM_G2_CHECK_SUBGROUP does.  Anything else gives meaningless points at the places that depend on it (after log_n stages: every place of
 *      its array), never a fault and never a change to another array of the batch: every address is a function of the lane index only.
 *      Stream-ordered on hip_stream (NULL = the context's stream): the call returns when enqueued.  The twiddle tables are the G1 transform's:
 *      one table per log_n >= 2 on the context serves both groups and both directions (msm_g2_fft_plan_t.table_bytes ==
 *      msm_g1_fft_plan_t.table_bytes), built on the stream of whichever call first needs it; a call on ANOTHER stream waits for the event behind
 *      that build.  A coset form is not offered (multiply by g^i with msm_bn254_g2_pointwise_mul_device), later stages do not skip their w = 1
 *      butterflies, and one call runs on one GPU.
 *      Errors, as for G1: a NULL or misaligned pointer, an unknown flag bit, log_n > 28, batch * n > 2^36, a bad base_form: MSM_ERR_BAD_ARG;
 *      batch == 0: MSM_ERR_EMPTY; allocation failure: MSM_ERR_OOM.  A failed call writes nothing and the context stays usable. ---- */
typedef struct {
    uint16_t stages;         /* butterfly launches per 2^30 butterflies: log_n */
    uint16_t ladder_stages;  /* ... of them with a scalar multiplication per butterfly: log_n - 1 (0 for log_n == 0) */
    uint32_t inv_group;      /* butterflies that share one field inversion (twice per ladder stage: the slopes' norms, the 2 * inv_group outputs) */
    uint64_t table_bytes;    /* kept on the context for this size, shared with the G1 transform: n / 2 twiddles of 32 bytes (0 below log_n = 2) */
} msm_g2_fft_plan_t;

/* host only, no context */
int32_t msm_bn254_g2_fft_plan(uint32_t log_n, msm_g2_fft_plan_t *out);
int32_t msm_bn254_g2_fft_device(msm_ctx *ctx, void *d_xy, void *d_inf, uint32_t log_n, size_t batch, uint32_t flags, void *hip_stream);
/* on host pointers, blocking.  base_form: MSM_FORM_STD / _MONT (MSM_PM_BASES_STD is not taken here); inf NULL: nothing is flagged; out_xy may be
 * xy and out_inf may be inf.  The whole batch is staged in device memory (129 bytes per point, kept on the context and shared with
 * msm_bn254_g1_fft): a transform cannot be chunked.  Pageable memory is pinned in place like every host-pointer call. */
int32_t msm_bn254_g2_fft(msm_ctx *ctx, const uint32_t *xy, uint32_t base_form, const uint8_t *inf, uint32_t log_n, size_t batch, uint32_t flags,
                         uint32_t *out_xy, uint8_t *out_inf);

/* ---- BN254 scalar field Fr: the scalars of a setup made in HBM (ABI 7) -- what the fixed-base calls above read as k_i:
 *      powers of tau (the H query, KZG), element-wise inverses, the Lagrange coefficients L_i(tau) of the transforms' domain, and the linear
 *      combination of the L query.  Conventions of msm_bn254_fr_ntt_device: elements are 8 little-endian words; any 256-bit input pattern is
 *      read modulo r; outputs are canonical (< r), so results are bit-exact; MSM_NTT_IN_MONT / MSM_NTT_OUT_MONT name the form of the DEVICE
 *      arrays (arkworks Fr.0; standard form by default).  tau, base, scale and the coefficients are HOST pointers to 8 standard-form words, read
 *      modulo r.  Device arrays are 16-byte aligned.  Stream-ordered on hip_stream (NULL = the context's stream): a call returns when enqueued.
 *      UNLIKE the transforms, these calls keep nothing on the context -- no table, no scratch array, no event; every constant travels with the
 *      kernel launch -- so two calls on two streams do NOT wait for each other, and the caller orders calls that share an array.
 *      Errors: a NULL or misaligned pointer, an unknown flag bit, n > 2^36: MSM_ERR_BAD_ARG; n == 0: MSM_ERR_EMPTY; allocation failure (host
 *      form): MSM_ERR_OOM.  The context stays usable after any of them. ---- */
typedef struct {
    uint32_t inv_group;            /* elements that share one field inversion (a chain of the inverse and Lagrange kernels) */
    uint32_t block_points;         /* consecutive elements one workgroup of those kernels covers: 256 * inv_group */
    uint32_t powers_block_points;  /* ... one workgroup of the powers kernel */
    uint32_t reserved;
} msm_fr_vector_plan_t;
/* host only, no context */
int32_t msm_bn254_fr_vector_plan(msm_fr_vector_plan_t *out);
/* out[i] = scale * base^(first + i), i < n.  scale_std NULL = 1.  0^0 = 1: base = 0 gives out[0] = scale when first == 0 and 0 elsewhere.
 * flags: MSM_NTT_OUT_MONT only.  first + n must not exceed 2^64.  About two field multiplications per element. */
int32_t msm_bn254_fr_powers_device(msm_ctx *ctx, const uint32_t *base_std, const uint32_t *scale_std, uint64_t first, void *d_out, size_t n,
                                   uint32_t flags, void *hip_stream);
/* out[i] = 1 / in[i]; an element = 0 (mod r) gives 0 and leaves its neighbours alone (arkworks' batch_inversion).  d_out may be d_in.  With
 * MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT x * 2^256 maps to x^-1 * 2^256.  One field inversion per inv_group elements. */
int32_t msm_bn254_fr_batch_inverse_device(msm_ctx *ctx, const void *d_in, void *d_out, size_t n, uint32_t flags, void *hip_stream);
/* host pointers, blocking; out == in allowed; stages through a device allocation of n * 32 bytes that is freed before the call returns */
int32_t msm_bn254_fr_batch_inverse(msm_ctx *ctx, const uint32_t *in, uint32_t *out, size_t n, uint32_t flags);
/* out[i] = L_i(tau) = Z(tau) w^i / (n (tau - w^i)), i < n = 2^log_n, Z(tau) = tau^n - 1, w = msm_bn254_fr_root_of_unity(log_n).  tau in the
 * domain gives the unit vector (1 where w^i = tau).  log_n == 0: out[0] = 1.  log_n > 28: MSM_ERR_BAD_ARG.  flags: MSM_NTT_OUT_MONT only. */
int32_t msm_bn254_fr_lagrange_device(msm_ctx *ctx, const uint32_t *tau_std, uint32_t log_n, void *d_out, uint32_t flags, void *hip_stream);
/* out[i] = ka * a[i] + kb * b[i] + kc * c[i].  d_b / d_c NULL: the term is dropped; a NULL coefficient is 1.  d_out may alias any input. */
int32_t msm_bn254_fr_lincomb_device(msm_ctx *ctx, const void *d_a, const uint32_t *ka_std, const void *d_b, const uint32_t *kb_std,
                                    const void *d_c, const uint32_t *kc_std, void *d_out, size_t n, uint32_t flags, void *hip_stream);

/* ---- BN254 scalar field Fr: scans (ABI 7) -- calls whose output element depends on EVERYTHING after or before it: the
 *      value of a polynomial at a point, its quotient by X - z (the proof of a KZG opening is the MSM of that quotient) and the running
 *      product (the grand product Z of PLONK and halo2).  Conventions of the Fr-vector section above: elements are 8 little-endian words; any
 *      256-bit input pattern is read modulo r; outputs are canonical (< r), so results are bit-exact; MSM_NTT_IN_MONT / MSM_NTT_OUT_MONT name
 *      the form of the DEVICE arrays; z is a HOST pointer to 8 standard-form words, read modulo r; device arrays are 16-byte aligned.
 *      Stream-ordered on hip_stream (NULL = the context's stream): a call returns when enqueued, and a single value (d_value, d_rem, d_total)
 *      is written to DEVICE memory.  A call is two (evaluation) or three kernel launches with a scratch array between them.
 *      UNLIKE the Fr vectors, this family keeps ONE array on the context: the aggregates of the workgroups (36 bytes per block_points elements,
 *      grown on demand, freed by msm_ctx_destroy).  The ordering rule is the transforms': every call leaves an event behind, and a call on
 *      ANOTHER stream than the previous one waits for it first.  The caller orders calls that share a data array.
 *      Errors: a NULL or misaligned pointer, an unknown flag bit, n > 2^36: MSM_ERR_BAD_ARG; n == 0: MSM_ERR_EMPTY; allocation failure:
 *      MSM_ERR_OOM.  A failed call has written nothing and the context stays usable. ---- */
#define MSM_FR_SCAN_EXCLUSIVE 32u /* msm_bn254_fr_running_product_device: out[0] = 1, out[i] = in[0] * .. * in[i - 1] (Z as PLONK stores it) */
typedef struct {
    uint32_t chain;          /* consecutive elements one lane folds */
    uint32_t block_points;   /* consecutive elements one workgroup covers: 256 * chain */
    uint32_t eval_launches;  /* kernel launches of msm_bn254_fr_poly_eval_device */
    uint32_t div_launches;   /* ... of msm_bn254_fr_poly_div_linear_device and of msm_bn254_fr_running_product_device */
    uint64_t blocks;         /* workgroups of the first and the last launch for n: ceil(n / block_points); the launch between is ONE workgroup
                              * that walks them in ceil(blocks / 256) rounds */
    uint64_t scratch_bytes;  /* kept on the context for n: 36 * blocks */
} msm_fr_scan_plan_t;
/* host only, no context (32 bytes: the library and tests/test_fr_scan_cpu.py assert the size).  n == 0: MSM_ERR_EMPTY; n > 2^36 or out NULL: MSM_ERR_BAD_ARG */
int32_t msm_bn254_fr_scan_plan(size_t n, msm_fr_scan_plan_t *out);
/* d_value[0..8) = sum_{i < n} c[i] * z^i. */
int32_t msm_bn254_fr_poly_eval_device(msm_ctx *ctx, const void *d_coeffs, size_t n, const uint32_t *z_std, void *d_value, uint32_t flags,
                                      void *hip_stream);
/* p(X) = q(X) * (X - z) + p(z):  d_quot receives n elements, q[j] = sum_{i > j} c[i] * z^(i - j - 1) for j < n - 1 and q[n - 1] = 0 (the array
 * keeps the length of the base set its MSM runs against); d_rem (8 words, may be NULL) receives p(z).  d_quot may be d_coeffs.  n == 1:
 * q[0] = 0 and the remainder is c[0].  z = 0 is an ordinary input (the quotient is the shift): nothing is inverted. */
int32_t msm_bn254_fr_poly_div_linear_device(msm_ctx *ctx, const void *d_coeffs, size_t n, const uint32_t *z_std, void *d_quot, void *d_rem,
                                            uint32_t flags, void *hip_stream);
/* host pointers, blocking; quot == coeffs allowed, rem may be NULL; stages through a device allocation of n * 32 + 32 bytes that is freed
 * before the call returns.  Pageable memory is pinned in place like every host-pointer call. */
int32_t msm_bn254_fr_poly_div_linear(msm_ctx *ctx, const uint32_t *coeffs, size_t n, const uint32_t *z_std, uint32_t *quot, uint32_t *rem,
                                     uint32_t flags);
/* out[i] = in[0] * .. * in[i]; with MSM_FR_SCAN_EXCLUSIVE out[0] = 1 and out[i] = in[0] * .. * in[i - 1].  d_total (8 words, may be NULL)
 * receives the product of all n elements in either mode.  d_out may be d_in.  An element = 0 (mod r) zeroes everything after it.
 * flags: MSM_NTT_IN_MONT, MSM_NTT_OUT_MONT, MSM_FR_SCAN_EXCLUSIVE. */
int32_t msm_bn254_fr_running_product_device(msm_ctx *ctx, const void *d_in, void *d_out, size_t n, void *d_total, uint32_t flags,
                                            void *hip_stream);

/* ---- introspection --------------------------------------------------------------------------- */
/* the plan of a call on n points under (window_bits, flags); with MSM_FLAG_WINDOW_TABLE in flags: the plan of a RESIDENT call on a
 * set of n bases uploaded under those flags (window width, table factor, table memory) */
int32_t msm_plan(size_t n, uint32_t window_bits, uint32_t flags, msm_plan_t *out);
int32_t msm_get_timings(const msm_ctx *ctx, msm_timings_t *out);
/* size-checked forms (ABI 7): at most out_size bytes are written -- a consumer built against an older, shorter msm_timings_t passes ITS
 * sizeof and is not overrun; fields beyond the library's struct are left untouched.  out_size == 0: MSM_ERR_BAD_ARG. */
int32_t msm_get_timings_sized(const msm_ctx *ctx, void *out, size_t out_size);
/* per-stage hipEvents are OFF by default (every record costs ~6 us of stream time); when off, the stage fields of
 * msm_timings_t other than accumulate_ms / finish_ms / total_ms read 0 */
int32_t msm_set_stage_timing(msm_ctx *ctx, int32_t enabled);
/* Which launches of the accumulate kernel carry their pair of hipEvents (ABI 7): every `every_n`-th one; 0 = none (the DEFAULT since ABI 7), 1 = all of them (what ABI <= 6 did).
 * The events ride on the kernel's dispatch, but a timed dispatch does not overlap its neighbours' launch latency: ~11 us per MSM at every size.  A caller
 * that reads msm_get_accumulate_kernel_stats / msm_timings_t.accumulate_ms turns them on; bench.py samples every 4th launch of its timed loop.
 * Stage timing (msm_set_stage_timing) times every launch whatever this says.  msm_timings_t.accumulate_ms reads 0 after an untimed launch. */
int32_t msm_set_kernel_timing(msm_ctx *ctx, uint32_t every_n);
/* average duration (ms) of the TIMED accumulate kernel launches since the last reset, measured with
 * hipEvents on the stream the kernel runs on; *launches receives their count */
int32_t msm_get_accumulate_kernel_stats(const msm_ctx *ctx, double *avg_ms, uint64_t *launches);
void msm_reset_kernel_stats(msm_ctx *ctx);
/* Clock probe of the accumulate kernel since the last reset (ABI 5): the first workgroup of every launch brackets its chunk with the
 * shader-cycle counter and the constant-rate counter.  *sclk_ghz = the shader clock the kernel really sustained (cycles / ticks x
 * hipDeviceAttributeWallClockRate); *cycles_per_addition = shader cycles that wavefront needed per mixed addition (three wavefronts
 * share a SIMD): equal on two boxes that execute the same instruction stream, whatever their clocks; *samples = launches sampled.
 * Any pointer may be NULL.  Synchronises the context's stream. */
int32_t msm_get_clock_stats(msm_ctx *ctx, double *sclk_ghz, double *cycles_per_addition, uint64_t *samples);

#ifdef __cplusplus
}
#endif
#endif /* MSM_HIP_H */
